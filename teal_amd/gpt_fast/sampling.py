"""Per-request sampling of the fused engines (teal_amd/csrc/teal_sample_rows.hip): the parameter rows an engine keeps per slot
and the one launch that draws every row's token under its own temperature, top_k, top_p and min_p.

Order of application: temperature, top_k (ties at the pivot kept), top_p over the renormalised top-k set (a value stays iff the
mass of the values strictly above it is below top_p of the set's; equal logits stay or go together, the maximum always stays),
min_p (a value stays iff its weight is at least min_p times the maximum's), then the fused sampler's exponential race over what
stayed.  The launch reads its parameters from device memory and is predicated per slot, so an admission changes a row without
re-capturing the step and one captured step serves any mix of settings.  With top_p = 1 and min_p = 0 a row draws the very token
the fused top-k sampler draws.
"""
from __future__ import annotations

import math
import struct
from typing import Dict, Optional

import torch

from .. import _lib, runtime
from .logit_processors import MAX_VOCAB, fp32

DEFAULT_ROW = (1.0, 0, 1.0, 0.0)  # temperature 1, no filter: a row nobody has set samples the model's own distribution


def check_sampling(temperature=0.8, top_k=None, top_p=1.0, min_p=0.0) -> Dict:
    """the four settings, validated (ValueError with the reason) and normalised to {temperature: float, top_k: int (0: off),
    top_p: float, min_p: float}.  Numbers are judged as the fp32 values the parameter row will hold."""
    def real(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not math.isfinite(fp32(v)):
            raise ValueError(f"{name} must be a finite number (in fp32), got {v!r}")
        return float(v)
    t = real("temperature", temperature)
    if t < 0.0:
        raise ValueError(f"temperature must be >= 0 (values below 1e-5 sample as 1e-5: the argmax), got {temperature!r}")
    if top_k is None:
        top_k = 0
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < 2 ** 31:
        raise ValueError(f"top_k must be a non-negative integer (0 or None: off), got {top_k!r}")
    p = real("top_p", top_p)
    if fp32(p) <= 0.0:
        raise ValueError(f"top_p must be > 0 in fp32 (1 or more: off), got {top_p!r}")
    m = real("min_p", min_p)
    if m < 0.0 or fp32(m) >= 1.0:
        raise ValueError(f"min_p must be in [0, 1) in fp32 (0: off), got {min_p!r}")
    return {"temperature": t, "top_k": int(top_k), "top_p": p, "min_p": m}


def row_words(c: Dict) -> torch.Tensor:
    """the four 32-bit words of a parameter row: {fp32 temperature, int32 top_k, fp32 top_p, fp32 min_p}"""
    raw = struct.pack("<fiff", c["temperature"], c["top_k"], c["top_p"], c["min_p"])
    return torch.tensor(struct.unpack("<4i", raw), dtype=torch.int32)


class SamplingParams:
    """params int32 [rows][4] (the words of {temperature, top_k, top_p, min_p}) and kept int32 [rows] (how many logits entered
    each row's last race) — on `device`, rows = the engine's slots"""

    def __init__(self, rows: int, vocab: int, dtype: torch.dtype, device):
        if vocab < 8 or vocab > MAX_VOCAB or vocab % 8:  # (refused here, not by the first launch in the middle of an admission)
            raise ValueError(f"per-request sampling needs a vocabulary that is a multiple of 8 in 8..{MAX_VOCAB} (the sampling launch's "
                             f"contract), got {vocab}")
        self.rows, self.vocab, self.dtype = int(rows), int(vocab), dtype
        d = check_sampling(*DEFAULT_ROW)
        self.params = row_words(d).repeat(rows, 1).to(device)
        self.kept = torch.zeros(rows, dtype=torch.int32, device=device)
        self.settings = [dict(d) for _ in range(rows)]  # the host's copy of what the rows hold
        self.code = runtime.dtype_code(dtype)
        self.L = _lib.load()

    def loop_tensors(self):
        """what a captured step writes (nothing is carried from replay to replay; a capture's warm-up step is undone on it)"""
        return (self.kept,)

    def set_row(self, row: int, temperature: float = 0.8, top_k: Optional[int] = None, top_p: float = 1.0, min_p: float = 0.0):
        if not 0 <= int(row) < self.rows:
            raise ValueError(f"slot {row} outside 0..{self.rows - 1}")
        c = check_sampling(temperature, top_k, top_p, min_p)
        self.params[row].copy_(row_words(c))
        self.settings[row] = c

    def launch(self, logits: torch.Tensor, stride: int, B: int, rng_state: torch.Tensor, tokens: torch.Tensor,
               pos: Optional[torch.Tensor], history: Optional[torch.Tensor], history_len: int, row0: int = 0,
               active: Optional[int] = None, st=None):
        """rows row0 .. row0+B-1 draw from `logits` row r (stride elements apart): rng_state [B][2], tokens [B], pos [B] or None,
        history [B][history_len] or None are row r's; `active`: the address of the slot engine's active word — row r is
        predicated on its bit row0 + r"""
        rc = self.L.teal_sample_rows(logits.data_ptr(), stride, self.vocab, self.code, B, self.params[row0].data_ptr(),
                                     rng_state.data_ptr(), tokens.data_ptr(), pos.data_ptr() if pos is not None else None,
                                     history.data_ptr() if history is not None else None, int(history_len),
                                     self.kept[row0:].data_ptr(), active, row0, runtime.stream_ptr() if st is None else st)
        if rc != 0:
            _lib.check(rc, "teal_sample_rows")
