"""Continuous batching: requests of different prompt lengths and budgets share the B <= 8 slots of one batched step.

A request is prompt token ids, a token budget and an optional EOS id.  The step (SlotDecodeEngine, teal_amd/gpt_fast/batched.py)
switches a finished slot off on the device, so a captured step replays unchanged whatever the active set; TEAL's rule stays
per sequence and a step reads the union of the rows the ACTIVE sequences keep.  Between bursts of `sync_every` replays the
host reads the slot state back in one copy, harvests the finished requests (their history rows) and admits waiting ones in FIFO
order, one dense prompt pass each.

refill="free" admits into every free slot; refill="all" only when every slot is free — static batching on the same engine
(the benchmark's baseline).  Request r draws from its own stream, seed + r (draw 0 is its first token, draw i decode step i),
so its tokens do not depend on its slot, on the requests beside it or on sync_every (where the union does not either: every
row kept).
"""
from __future__ import annotations

import json
import time
from collections import deque
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

from .batched import SLOT_ACTIVE, SLOT_FINISH, SLOT_PRODUCED, SLOT_STEP

REFILL = ("free", "all")


@dataclass
class Request:
    tokens: List[int]
    max_new_tokens: int
    eos_id: Optional[int] = None
    seed: Optional[int] = None  # its random stream; None: the batcher's seed + its index


def parse_requests(lines: Sequence[str], default_max_new_tokens: int, tokenizer=None, eos_id: Optional[int] = None) -> List[Request]:
    """JSON Lines, one request per line: {"tokens": [...]} or {"prompt": "..."} (needs a tokenizer; BOS prepended as generate.py
    does), with an optional "max_new_tokens" (default: `default_max_new_tokens`).  Blank lines are skipped."""
    out = []
    for i, line in enumerate(lines):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
        except json.JSONDecodeError as e:
            raise ValueError(f"request line {i + 1}: not JSON ({e})") from None
        if not isinstance(d, dict) or ("tokens" in d) == ("prompt" in d):
            raise ValueError(f"request line {i + 1}: needs exactly one of \"tokens\" and \"prompt\"")
        if "tokens" in d:
            toks = d["tokens"]
            if not isinstance(toks, list) or not toks or not all(isinstance(t, int) and t >= 0 for t in toks):
                raise ValueError(f"request line {i + 1}: \"tokens\" must be a non-empty list of token ids")
        else:
            if tokenizer is None:
                raise ValueError(f"request line {i + 1}: a \"prompt\" needs a tokenizer (a checkpoint), not --synthetic")
            toks = [tokenizer.bos_id()] + tokenizer.encode(d["prompt"])
        n = d.get("max_new_tokens", default_max_new_tokens)
        if not isinstance(n, int) or n < 1:
            raise ValueError(f"request line {i + 1}: \"max_new_tokens\" must be a positive integer")
        out.append(Request([int(t) for t in toks], n, eos_id))
    if not out:
        raise ValueError("no requests")
    return out


def cache_rows(requests: Sequence[Request], block_size: int) -> int:
    """the cache length a run needs: the longest prompt + budget, capped at block_size; a request that cannot fit is refused"""
    for i, r in enumerate(requests):
        if len(r.tokens) + r.max_new_tokens > block_size:
            raise ValueError(f"request {i}: {len(r.tokens)} prompt tokens + {r.max_new_tokens} new tokens exceed the model's "
                             f"block_size {block_size}")
    return min(max(len(r.tokens) + r.max_new_tokens for r in requests), block_size)


class ContinuousBatcher:
    """Runs requests through an engine with B slots.  The engine offers B, max_seq, admit(slot, tokens, budget, eos_id, seed,
    temperature, top_k), run_steps(k, temperature, top_k, use_graph), read_state() (the slot state words, one copy),
    read_history(slot, n) and union_kept()."""

    def __init__(self, engine, sync_every: int = 8, refill: str = "free", temperature: float = 0.8, top_k: Optional[int] = 200,
                 seed: int = 1234, use_graph: bool = True):
        if refill not in REFILL:
            raise ValueError(f"refill must be one of {REFILL}")
        if int(sync_every) < 1:
            raise ValueError("sync_every must be >= 1")
        self.eng, self.K, self.refill = engine, int(sync_every), refill
        self.temperature, self.top_k, self.seed, self.use_graph = temperature, top_k, int(seed), use_graph

    def _clock(self):
        try:
            import torch
            if torch.cuda.is_available():
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                return e
        except ImportError:
            pass
        return time.perf_counter()

    @staticmethod
    def _seconds(a, b) -> float:
        return (b - a) if isinstance(a, float) else a.elapsed_time(b) / 1000.0

    def run(self, requests: Sequence[Request]) -> Dict:
        eng, B = self.eng, self.eng.B
        for i, r in enumerate(requests):  # refused before anything runs
            if len(r.tokens) < 1 or r.max_new_tokens < 1 or len(r.tokens) + r.max_new_tokens > eng.max_seq:
                raise ValueError(f"request {i}: {len(r.tokens)} prompt tokens + {r.max_new_tokens} new tokens do not fit a cache of "
                                 f"{eng.max_seq} rows")
        pending = deque(range(len(requests)))
        slot_req: List[Optional[int]] = [None] * B
        admitted_at = [0] * B
        out: List[Optional[List[int]]] = [None] * len(requests)
        slots_used: List[int] = [-1] * len(requests)
        steps = admissions = slot_steps = 0
        step0 = eng.read_state()[SLOT_STEP]  # the engine's step counter (finish steps are on its scale)
        admit_spans = []
        t0 = time.perf_counter()
        c0 = self._clock()
        while pending or any(r is not None for r in slot_req):
            free = [s for s in range(B) if slot_req[s] is None]
            if pending and free and (self.refill == "free" or len(free) == B):
                a0 = self._clock()
                for s in free:
                    if not pending:
                        break
                    r = pending.popleft()
                    q = requests[r]
                    eng.admit(s, q.tokens, q.max_new_tokens, q.eos_id, self.seed + r if q.seed is None else q.seed, self.temperature,
                              self.top_k)
                    slot_req[s], admitted_at[s], slots_used[r] = r, step0 + steps, s
                    admissions += 1
                admit_spans.append((a0, self._clock()))
            eng.run_steps(self.K, self.temperature, self.top_k, self.use_graph)
            steps += self.K
            state = eng.read_state()
            for s in range(B):
                r = slot_req[s]
                if r is None or (state[SLOT_ACTIVE] >> s) & 1:
                    continue
                out[r] = eng.read_history(s, state[SLOT_PRODUCED + s])
                slot_steps += state[SLOT_FINISH + s] - admitted_at[s]
                slot_req[s] = None
        c1 = self._clock()
        if not isinstance(c1, float):
            c1.synchronize()
        wall = time.perf_counter() - t0
        wall_dev = self._seconds(c0, c1)
        t_admit = sum(self._seconds(a, b) for a, b in admit_spans)
        useful = sum(len(o) for o in out)
        return {
            "tokens": out, "slots": slots_used, "steps": steps, "admissions": admissions, "wall_s": wall,
            "admission_s": t_admit, "admission_share": t_admit / wall_dev if wall_dev > 0 else 0.0,
            "mean_active_slots": slot_steps / steps if steps else 0.0, "useful_tokens": useful,
            "useful_tokens_per_sec": useful / wall if wall > 0 else 0.0, "union_kept": eng.union_kept(),
            "refill": self.refill, "sync_every": self.K, "batch_size": B,
        }
