"""Constrained decoding of continuous batching (teal_amd/csrc/teal_constrain.hip): token automata, the arena their images live
in, and the one launch that steps each slot's automaton and masks the row its sampler reads.

A token automaton has S >= 1 states, state 0 the start.  State s has `edges` — (token, next) pairs, tokens strictly ascending —, a
`default` and an `accept` flag; delta(s, t) is the `next` of the edge that names t, else the default, and t is allowed in s iff
delta(s, t) >= 0 (an edge with next = -1 is an exception to a non-negative default: "anything but these").  The request's EOS id
is open exactly in accepting states and never moves the automaton.  The state advances on the device inside the captured step,
read from device memory, so one captured graph serves any mix of requests — a host-side mask would only act every sync_every
steps, and every token drawn in between would be drawn unconstrained.

The match is on TOKEN IDS, not text: a string the model could spell with other tokens than the ones listed is not reachable.
Compilers from a regex or a JSON schema to an automaton are out of scope: `Automaton` takes explicit tables, so they can be added
on the host.  A banned logit becomes -MAXF (the dtype's most negative finite value); its weight in the samplers' race is exactly 0
while the temperature is at most MAX_TEMPERATURE, so admission refuses a constrained request above it.  Logprobs stay the model's
own: they are computed from the raw logits, not from the masked row.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib, runtime
from .logit_processors import MAX_VOCAB

VIOLATION, STATE_MASK = 1 << 30, 0x3FFFFFFF  # include/teal_hip.h, TEAL_CONSTRAIN_*
MAX_STATES = 2 ** 30 - 1
MAX_TEMPERATURE = 100.0  # above it expf((-MAXF - mx) / T) is no longer exactly 0 in fp16
ALIGN = 4  # arena blocks start on 16 bytes


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


class Automaton:
    """states: a sequence of {"edges": [(token, next), ...], "default": int (-1: none), "accept": bool}"""

    def __init__(self, states: Sequence[Dict]):
        if isinstance(states, (str, bytes, dict)) or not hasattr(states, "__iter__"):
            raise ValueError("an automaton takes a list of states")
        self.states: List[Dict] = []
        for s, st in enumerate(states):
            if not isinstance(st, dict):
                raise ValueError(f"state {s} must be an object with \"edges\", \"default\" and \"accept\"")
            edges = st.get("edges", ())
            if isinstance(edges, (str, bytes, dict)) or not hasattr(edges, "__iter__"):
                raise ValueError(f"state {s}: \"edges\" must be a list of [token, next] pairs")
            pairs = []
            for e in edges:
                if isinstance(e, (str, bytes)) or not hasattr(e, "__len__") or len(e) != 2 or not _is_int(e[0]) or not _is_int(e[1]):
                    raise ValueError(f"state {s}: an edge must be a [token, next] pair of integers, got {e!r}")
                pairs.append((int(e[0]), int(e[1])))
            d, a = st.get("default", -1), st.get("accept", False)
            if not _is_int(d):
                raise ValueError(f"state {s}: \"default\" must be an integer (-1: none), got {d!r}")
            if not isinstance(a, bool) and a not in (0, 1):
                raise ValueError(f"state {s}: \"accept\" must be true or false, got {a!r}")
            self.states.append({"edges": pairs, "default": int(d), "accept": bool(a)})
        if not self.states:
            raise ValueError("an automaton needs at least one state (state 0 is the start)")

    def __len__(self) -> int:
        return len(self.states)

    # ---- the rule on the host ----------------------------------------------------------------------------------------------
    def delta(self, s: int, t: int) -> int:
        st = self.states[s]
        for tok, nxt in st["edges"]:
            if tok == t:
                return nxt
        return st["default"]

    def check(self, vocab: int, eos_id: Optional[int], eos_known: bool = True) -> "Automaton":
        """ValueError with the reason for everything the device does not check: tokens unsorted, duplicated or outside the vocabulary,
        a `next` or `default` outside -1 .. S-1, an edge on the request's EOS id, a dead end — a state with no allowed token that
        is not accepting, or is accepting while the request has no EOS id —, more than 2^30 - 1 states.  Unreachable states are
        legal.  eos_known=False (a registration, before any request): the two rules that depend on the EOS id are left to the
        admission's check."""
        S = len(self.states)
        if S > MAX_STATES:
            raise ValueError(f"{S} states: at most 2^30 - 1 (the trace word's bits 30 and 31 are flags)")
        eos = None if eos_id is None or int(eos_id) < 0 else int(eos_id)
        for s, st in enumerate(self.states):
            last, banned, open_edges = -1, 0, 0
            for tok, nxt in st["edges"]:
                if not 0 <= tok < vocab:
                    raise ValueError(f"state {s}: token {tok} is outside the vocabulary 0..{vocab - 1}")
                if tok <= last:
                    raise ValueError(f"state {s}: tokens must be strictly ascending (token {tok} after {last}: " +
                                     ("duplicated)" if tok == last else "unsorted)"))
                last = tok
                if not -1 <= nxt < S:
                    raise ValueError(f"state {s}: next {nxt} of token {tok} is outside -1..{S - 1}")
                if eos is not None and tok == eos:
                    raise ValueError(f"state {s}: an edge names the request's EOS id {eos} (it is open exactly in accepting states)")
                banned += nxt < 0
                open_edges += nxt >= 0
            if not -1 <= st["default"] < S:
                raise ValueError(f"state {s}: default {st['default']} is outside -1..{S - 1}")
            allowed = open_edges if st["default"] < 0 else vocab - banned - (1 if eos is not None and eos < vocab else 0)
            if allowed <= 0 and not st["accept"]:
                raise ValueError(f"state {s} is a dead end: no token is allowed and it is not accepting")
            if allowed <= 0 and eos is None and eos_known:
                raise ValueError(f"state {s} is a dead end: no token is allowed and the request has no EOS id to end on")
        return self

    def image(self) -> List[int]:
        """the int32 words the launch reads: S header rows {edge_begin, edge_end, default, accept} with offsets relative to the
        image, then the edges as (token, next) pairs"""
        S = len(self.states)
        head, tail, at = [], [], 4 * S
        for st in self.states:
            n = 2 * len(st["edges"])
            head += [at, at + n, st["default"], int(st["accept"])]
            for tok, nxt in st["edges"]:
                tail += [tok, nxt]
            at += n
        return head + tail

    # ---- builders ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_choices(cls, choices: Sequence[Sequence[int]]) -> "Automaton":
        """a trie over token-id lists: the request produces exactly one of them (then its EOS id).  Leaves and complete prefixes
        accept; duplicates merge; an empty choice (or no choice) is refused"""
        if isinstance(choices, (str, bytes)) or not hasattr(choices, "__iter__"):
            raise ValueError("choices must be a list of token id lists")
        kids: List[Dict[int, int]] = [{}]
        accept = [False]
        n = 0
        for q, ch in enumerate(choices):
            if isinstance(ch, (str, bytes)) or not hasattr(ch, "__iter__"):
                raise ValueError(f"choice {q} must be a list of token ids, got {ch!r}")
            ch = list(ch)
            if not ch:
                raise ValueError(f"choice {q} is empty")
            s = 0
            for t in ch:
                if not _is_int(t) or t < 0:
                    raise ValueError(f"choice {q}: {t!r} is not a token id")
                if t not in kids[s]:
                    kids[s][t] = len(kids)
                    kids.append({})
                    accept.append(False)
                s = kids[s][t]
            accept[s] = True
            n += 1
        if not n:
            raise ValueError("choices is empty")
        return cls([{"edges": sorted(k.items()), "default": -1, "accept": a} for k, a in zip(kids, accept)])

    @classmethod
    def from_allowed(cls, ids: Sequence[int]) -> "Automaton":
        """one accepting state with a self-loop on every id: any sequence over `ids`, of any length"""
        if isinstance(ids, (str, bytes)) or not hasattr(ids, "__iter__"):
            raise ValueError("allowed_token_ids must be a list of token ids")
        ids = list(ids)
        if not ids or not all(_is_int(t) and t >= 0 for t in ids):
            raise ValueError("allowed_token_ids must be a non-empty list of token ids")
        return cls([{"edges": [(t, 0) for t in sorted(set(ids))], "default": -1, "accept": True}])

    def to_json(self) -> Dict:
        return {"states": [{"edges": [[t, n] for t, n in st["edges"]], "default": st["default"], "accept": st["accept"]} for st in self.states]}

    @classmethod
    def from_json(cls, d: Dict) -> "Automaton":
        if not isinstance(d, dict) or not isinstance(d.get("states"), list):
            raise ValueError("an automaton object needs \"states\": a list of {\"edges\", \"default\", \"accept\"}")
        return cls(d["states"])


class ArenaAllocator:
    """host free list over `capacity` words: first fit, blocks rounded up to ALIGN words, neighbours coalesced on release"""

    def __init__(self, capacity: int):
        if int(capacity) < ALIGN:
            raise ValueError(f"an arena needs at least {ALIGN} words, got {capacity}")
        self.capacity = int(capacity) // ALIGN * ALIGN
        self.free: List[Tuple[int, int]] = [(0, self.capacity)]  # (offset, words), ascending, never adjacent
        self.used: Dict[int, int] = {}

    def alloc(self, words: int) -> int:
        n = (max(int(words), 1) + ALIGN - 1) // ALIGN * ALIGN
        for i, (off, size) in enumerate(self.free):
            if size >= n:
                if size == n:
                    del self.free[i]
                else:
                    self.free[i] = (off + n, size - n)
                self.used[off] = n
                return off
        raise MemoryError(f"the constraint arena is full: {words} words asked, the largest free block has "
                          f"{max((s for _, s in self.free), default=0)} of {self.capacity}")

    def release(self, off: int):
        n = self.used.pop(off)
        self.free.append((off, n))
        self.free.sort()
        merged: List[Tuple[int, int]] = []
        for o, s in self.free:
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + s)
            else:
                merged.append((o, s))
        self.free = merged


class Constraints:
    """con [rows][vocab] (what the samplers read), table int32 [rows][4] = {base, S, 0, 0} (base -1: unconstrained), trace int32
    [rows][trace_len] (entry c: the state draw c was made in) and the arena int32 [capacity_words] at a fixed address — on `device`,
    rows = the engine's slots.  An image is shared by every slot that names it."""

    def __init__(self, rows: int, vocab: int, dtype: torch.dtype, trace_len: int, device, capacity_words: int = 1 << 20):
        if vocab < 8 or vocab > MAX_VOCAB or vocab % 8:
            raise ValueError(f"constraints need a vocabulary that is a multiple of 8 in 8..{MAX_VOCAB} (the constrain launch's contract), "
                             f"got {vocab}")
        if int(trace_len) < 1:
            raise ValueError("trace_len must be >= 1")
        self.rows, self.vocab, self.dtype, self.trace_len = int(rows), int(vocab), dtype, int(trace_len)
        self.alloc = ArenaAllocator(capacity_words)
        self.con = torch.zeros(rows, vocab, dtype=dtype, device=device)
        self.table = torch.tensor([[-1, 0, 0, 0]] * rows, dtype=torch.int32).to(device)
        self.trace = torch.zeros(rows, self.trace_len, dtype=torch.int32, device=device)
        self.arena = torch.zeros(self.alloc.capacity, dtype=torch.int32, device=device)
        self.images: Dict[str, Tuple[int, int, Automaton]] = {}  # name -> (base, S, automaton)
        self.row_names: List[Optional[str]] = [None] * self.rows  # the host's copy of what the table rows name
        self.code = runtime.dtype_code(dtype)
        self.L = _lib.load()

    def loop_tensors(self):
        """what a captured step writes (a capture's warm-up step is undone on it)"""
        return (self.trace,)

    def register(self, name: str, automaton: Automaton) -> int:
        """the automaton's image into the arena under `name`; returns its word offset.  The caller has run `check`."""
        if not isinstance(name, str) or not name:
            raise ValueError("a constraint's name must be a non-empty string")
        if name in self.images:
            raise ValueError(f"constraint {name!r} is registered already")
        words = automaton.image()
        base = self.alloc.alloc(len(words))
        self.arena[base:base + len(words)].copy_(torch.tensor(words, dtype=torch.int32))
        self.images[name] = (base, len(automaton), automaton)
        return base

    def drop(self, name: str):
        if name not in self.images:
            raise ValueError(f"unknown constraint {name!r}")
        users = [r for r, n in enumerate(self.row_names) if n == name]
        if users:
            raise RuntimeError(f"constraint {name!r} is in use by slot{'s' if len(users) > 1 else ''} {', '.join(map(str, users))}")
        self.alloc.release(self.images.pop(name)[0])

    def automaton(self, name: str) -> Automaton:
        if name not in self.images:
            raise ValueError(f"unknown constraint {name!r} (register_constraint first)")
        return self.images[name][2]

    def set_row(self, row: int, name: Optional[str]):
        """slot `row` follows constraint `name` from its next draw 0 on; None: unconstrained"""
        if not 0 <= int(row) < self.rows:
            raise ValueError(f"slot {row} outside 0..{self.rows - 1}")
        if name is not None and name not in self.images:
            raise ValueError(f"unknown constraint {name!r} (register_constraint first)")
        base, S = (-1, 0) if name is None else self.images[name][:2]
        self.table[row].copy_(torch.tensor([base, S, 0, 0], dtype=torch.int32))
        self.row_names[int(row)] = name

    def launch(self, logits: torch.Tensor, stride: int, B: int, tokens: torch.Tensor, rng_state: torch.Tensor, eos: int, row0: int = 0,
               active: Optional[int] = None, st=None):
        """rows row0 .. row0+B-1: `logits` row r (stride elements apart) -> con[row0 + r] under slot row0 + r's automaton; tokens
        [B]: what the step was fed; rng_state [B][2]: the draw counters; eos: the ADDRESS of slot row0's EOS word (int32 [B])"""
        rc = self.L.teal_constrain_logits(logits.data_ptr(), stride, self.vocab, self.code, B, tokens.data_ptr(), rng_state.data_ptr(), eos,
                                          self.table[row0].data_ptr(), self.arena.data_ptr(), self.arena.numel(),
                                          self.trace[row0].data_ptr(), self.trace_len, self.con[row0].data_ptr(), self.vocab, active, row0,
                                          runtime.stream_ptr() if st is None else st)
        if rc != 0:
            _lib.check(rc, "teal_constrain_logits")

    def read_trace(self, row: int, n: int) -> List[int]:
        """the trace words of draws 0 .. n-1 of the request in slot `row`: the state each draw was made in (bit 30: a violation)"""
        return self.trace[int(row), :int(n)].tolist()
