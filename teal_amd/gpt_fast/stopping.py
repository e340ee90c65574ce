"""Per-request stop conditions of continuous batching (teal_amd/csrc/teal_stop.hip): the table of stop rows a slot engine keeps
and the retire launch that reads it.

A request may end on any of up to 16 stop ids, on any of up to 8 stop sequences of up to 8 tokens each, on its budget or on the end
of its cache; `min_new_tokens` holds the stop ids, the slot's EOS id and the stop sequences back until that many tokens are
produced (the budget and the cache end are not held back).  The match happens on the device, inside the captured step, on TOKEN
IDS: a sequence is compared with the tokens the request generated — never with its prompt — and a text the model spells with
other tokens than the ones given is not caught.  The tokens that stop a request stay in its output, as an EOS id does.  The launch
records why a slot ended (REASON) and what matched (MATCH: the token id, or the sequence's index).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import _lib, runtime

# the stop row (include/teal_hip.h, TEAL_STOP_*): word offsets and limits
STOP_MIN, STOP_NIDS, STOP_NSEQ, STOP_REASON, STOP_MATCH, STOP_IDS, STOP_SEQLEN, STOP_SEQ, STOP_WORDS = 0, 1, 2, 3, 4, 8, 24, 32, 96
MAX_IDS, MAX_SEQS, MAX_SEQ_LEN, ROWS = 16, 8, 8, 8
RUNNING, STOP_TOKEN, STOP_SEQUENCE, LENGTH, CACHE = 0, 1, 2, 3, 4
REASONS = {RUNNING: None, STOP_TOKEN: "stop_token", STOP_SEQUENCE: "stop_sequence", LENGTH: "length", CACHE: "cache"}


def _is_id(t) -> bool:
    return isinstance(t, int) and not isinstance(t, bool)


def check_stops(vocab: int, stop_token_ids=(), stop_sequences=(), min_new_tokens=0) -> Dict:
    """the three settings, validated (ValueError with the reason) and normalised to {stop_token_ids: list (duplicates dropped,
    order kept), stop_sequences: list of lists, min_new_tokens: int}.  A one-token sequence is legal and stays a sequence."""
    if stop_token_ids is None:
        stop_token_ids = ()
    if stop_sequences is None:
        stop_sequences = ()
    if isinstance(stop_token_ids, (str, bytes)) or not hasattr(stop_token_ids, "__iter__"):
        raise ValueError(f"stop_token_ids must be a list of token ids, got {stop_token_ids!r}")
    ids: List[int] = []
    for t in stop_token_ids:
        if not _is_id(t) or not 0 <= t < vocab:
            raise ValueError(f"stop token id {t!r} is outside the vocabulary 0..{vocab - 1}")
        if t not in ids:
            ids.append(int(t))
    if len(ids) > MAX_IDS:
        raise ValueError(f"{len(ids)} stop token ids: at most {MAX_IDS} per request")
    if isinstance(stop_sequences, (str, bytes)) or not hasattr(stop_sequences, "__iter__"):
        raise ValueError(f"stop_sequences must be a list of token id lists, got {stop_sequences!r}")
    seqs: List[List[int]] = []
    for q, seq in enumerate(stop_sequences):
        if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
            raise ValueError(f"stop sequence {q} must be a list of token ids, got {seq!r}")
        seq = list(seq)
        if not seq:
            raise ValueError(f"stop sequence {q} is empty")
        if len(seq) > MAX_SEQ_LEN:
            raise ValueError(f"stop sequence {q} has {len(seq)} tokens: at most {MAX_SEQ_LEN}")
        for t in seq:
            if not _is_id(t) or not 0 <= t < vocab:
                raise ValueError(f"stop sequence {q}: token id {t!r} is outside the vocabulary 0..{vocab - 1}")
        seqs.append([int(t) for t in seq])
    if len(seqs) > MAX_SEQS:
        raise ValueError(f"{len(seqs)} stop sequences: at most {MAX_SEQS} per request")
    if not _is_id(min_new_tokens) or not 0 <= min_new_tokens < 2 ** 31:
        raise ValueError(f"min_new_tokens must be a non-negative integer, got {min_new_tokens!r}")
    return {"stop_token_ids": ids, "stop_sequences": seqs, "min_new_tokens": int(min_new_tokens)}


def is_default(c: Dict) -> bool:
    """no stop id, no stop sequence, no minimum: what a request that asks for nothing carries"""
    return not c["stop_token_ids"] and not c["stop_sequences"] and not c["min_new_tokens"]


def pack_row(c: Dict) -> List[int]:
    """the TEAL_STOP_WORDS words of a checked setting; REASON running, MATCH -1, unused id and sequence words -1"""
    row = [0] * STOP_WORDS
    row[STOP_MIN], row[STOP_NIDS], row[STOP_NSEQ] = c["min_new_tokens"], len(c["stop_token_ids"]), len(c["stop_sequences"])
    row[STOP_REASON], row[STOP_MATCH] = RUNNING, -1
    row[STOP_IDS:STOP_IDS + MAX_IDS] = c["stop_token_ids"] + [-1] * (MAX_IDS - len(c["stop_token_ids"]))
    for q in range(MAX_SEQS):
        seq = c["stop_sequences"][q] if q < len(c["stop_sequences"]) else []
        row[STOP_SEQLEN + q] = len(seq)
        row[STOP_SEQ + MAX_SEQ_LEN * q:STOP_SEQ + MAX_SEQ_LEN * (q + 1)] = seq + [-1] * (MAX_SEQ_LEN - len(seq))
    return row


class StopConditions:
    """table int32 [8][TEAL_STOP_WORDS] on `device`, row s for slot s, and the launch that retires by it"""

    def __init__(self, rows: int, vocab: int, device):
        if not 1 <= int(rows) <= ROWS:
            raise ValueError(f"stop conditions serve 1..{ROWS} slots, got {rows}")
        self.rows, self.vocab = int(rows), int(vocab)
        empty = pack_row(check_stops(self.vocab))
        self.table = torch.tensor([empty] * ROWS, dtype=torch.int32).to(device)
        self._host = torch.zeros(ROWS, STOP_WORDS, dtype=torch.int32)
        self.settings = [check_stops(self.vocab) for _ in range(ROWS)]  # the host's copy of what the rows hold
        self.L = _lib.load()

    def loop_tensors(self):
        """what a captured step writes (REASON and MATCH of a slot it stops; a capture's warm-up step is undone on it)"""
        return (self.table,)

    def set_row(self, row: int, stop_token_ids=(), stop_sequences=(), min_new_tokens=0):
        """slot `row` starts over under these settings: REASON running, MATCH -1"""
        if not 0 <= int(row) < self.rows:
            raise ValueError(f"slot {row} outside 0..{self.rows - 1}")
        c = check_stops(self.vocab, stop_token_ids, stop_sequences, min_new_tokens)
        self.table[row].copy_(torch.tensor(pack_row(c), dtype=torch.int32))
        self.settings[row] = c

    def launch(self, slot_state: int, tokens: torch.Tensor, pos: torch.Tensor, history: torch.Tensor, B: int, mask: int, max_seq: int,
               count_step: bool, st=None):
        """teal_batched_retire_stops over slots 0 .. B-1 in `mask`: slot_state the address of the engine's slot words, tokens [B],
        pos [B], history [B][stride] with stride > the tokens a request can produce"""
        rc = self.L.teal_batched_retire_stops(slot_state, tokens.data_ptr(), pos.data_ptr(), history.data_ptr(), history.shape[-1],
                                              self.table.data_ptr(), B, mask, max_seq, int(count_step),
                                              runtime.stream_ptr() if st is None else st)
        if rc != 0:
            _lib.check(rc, "teal_batched_retire_stops")

    def read(self) -> List[Tuple[Optional[str], int]]:
        """(reason name — None while the slot runs —, match) per slot, in one device-to-host copy"""
        self._host.copy_(self.table)
        rows = self._host[:, [STOP_REASON, STOP_MATCH]].tolist()
        return [(REASONS.get(r), m) for r, m in rows][:self.rows]

