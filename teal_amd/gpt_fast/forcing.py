"""Teacher-forced tokens of continuous batching (teal_amd/csrc/teal_force.hip): the table of tokens a slot engine's requests were
told to take, and the one launch that puts them in the place of the tokens their samplers drew.

A request may carry forced tokens: its draws 0 .. n-1 do not yield what the sampler drew but the n tokens it was given.  The launch
follows a draw's sampler launch or launches and precedes the logprob and retire launches, inside the captured step, so a forced
token is the drawn token for everything behind it: its logprob is the model's log p(token | everything before it) — what scoring
a given continuation needs —, the retire launch counts and matches it, the next step is fed it and the next step's logit
processors count it.  The sampler still runs for a forced row (its draw is overwritten): the draw counter moves as for any draw,
so a request that goes on after its last forced token draws what it would have drawn had it sampled those tokens itself.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import _lib, runtime

ROWS = 8  # rows of the table = the slots of a step


def _is_id(t) -> bool:
    return isinstance(t, int) and not isinstance(t, bool)


def check_forced(vocab: int, forced_tokens=()) -> List[int]:
    """a request's forced tokens, validated (ValueError with the reason) -> a list of ints; None and () are "none" """
    if forced_tokens is None:
        return []
    if isinstance(forced_tokens, (str, bytes, dict)) or not hasattr(forced_tokens, "__iter__"):
        raise ValueError(f"forced_tokens must be a list of token ids, got {forced_tokens!r}")
    out = []
    for t in forced_tokens:
        if not _is_id(t) or not 0 <= t < vocab:
            raise ValueError(f"forced token id {t!r} is outside the vocabulary 0..{vocab - 1}")
        out.append(int(t))
    return out


class ForcedTokens:
    """table int32 [8][capacity] and lengths int32 [8] on `device`, row s for slot s, and the launch that reads them.  Only
    admissions write them (set_row), between replays: a captured step carries nothing of theirs from replay to replay."""

    def __init__(self, rows: int, capacity: int, vocab: int, device):
        if not 1 <= int(rows) <= ROWS:
            raise ValueError(f"forced tokens serve 1..{ROWS} slots, got {rows}")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"the forced-token capacity must be a positive integer, got {capacity!r}")
        self.rows, self.capacity, self.vocab = int(rows), int(capacity), int(vocab)
        self.table = torch.zeros(ROWS, self.capacity, dtype=torch.int32, device=device)
        self.lengths = torch.zeros(ROWS, dtype=torch.int32, device=device)
        self.L = _lib.load()

    def set_row(self, row: int, forced_tokens=()):
        """slot `row` starts over: its length word, then the row's first len entries (the rest keep what they held: never read)"""
        if not 0 <= int(row) < self.rows:
            raise ValueError(f"slot {row} outside 0..{self.rows - 1}")
        toks = check_forced(self.vocab, forced_tokens)
        if len(toks) > self.capacity:
            raise ValueError(f"{len(toks)} forced tokens: the table holds {self.capacity} per request (set_forced_tokens(capacity=))")
        self.lengths[row:row + 1].copy_(torch.tensor([len(toks)], dtype=torch.int32))
        if toks:
            self.table[row, :len(toks)].copy_(torch.tensor(toks, dtype=torch.int32))

    def launch(self, rows: int, rng_state: torch.Tensor, tokens: torch.Tensor, history: Optional[torch.Tensor], history_len: int,
               row0: int = 0, active: Optional[int] = None, st=None):
        """rows row0 .. row0+rows-1: draw counter rng_state[r][1], token tokens[r], history row r (history_len entries apart) —
        the first row's; `active`: the address of the slot engine's active word — row r is predicated on its bit row0 + r"""
        rc = self.L.teal_force_tokens(self.table[row0].data_ptr(), self.capacity, self.lengths[row0:].data_ptr(), rng_state.data_ptr(),
                                      tokens.data_ptr(), history.data_ptr() if history is not None else None, history_len, rows, active,
                                      row0, runtime.stream_ptr() if st is None else st)
        if rc != 0:
            _lib.check(rc, "teal_force_tokens")

    def read(self, row: int) -> int:
        """the length word of slot `row`"""
        return int(self.lengths[row].item())
