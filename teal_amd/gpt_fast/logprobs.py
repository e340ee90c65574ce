"""Token log-probabilities of the fused engines (teal_amd/csrc/teal_logprob.hip): the buffers an engine records into and the one
launch that fills them.

A logprob here is the MODEL's: log softmax of the step's 16-bit logits at temperature 1 with no top-k filter, whatever the
sampler that drew the token was told.  The launch follows a step's sampler launches and files each row's results under the draw
its sampler has just counted, so entry i of a row belongs to the token history[i] of that row; it lives inside the captured step,
so nothing leaves the hipGraph.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib, runtime

MAX_TOP = 8


def check_setting(n) -> Optional[int]:
    """None (off), 0 (the chosen token's logprob only) or 1..8 (that many alternates as well)"""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_TOP:
        raise ValueError(f"logprobs must be None (off) or an integer in 0..{MAX_TOP} (alternates per token), got {n!r}")
    return n


class LogprobBuffers:
    """lp [rows][length], top_ids / top_lp [rows][length][top_n] on `device` (top_n = 0: no alternates)"""

    def __init__(self, rows: int, length: int, top_n: int, device):
        self.rows, self.length, self.top_n = int(rows), int(length), int(top_n)
        self.lp = torch.zeros(rows, length, dtype=torch.float32, device=device)
        self.top_ids = torch.zeros(rows, length, top_n, dtype=torch.int32, device=device)
        self.top_lp = torch.zeros(rows, length, top_n, dtype=torch.float32, device=device)
        self.L = _lib.load()

    def tensors(self):
        return (self.lp, self.top_ids, self.top_lp)

    def launch(self, logits: torch.Tensor, stride: int, vocab: int, code: int, B: int, tokens: torch.Tensor, rng_state: torch.Tensor,
               row0: int = 0, active: Optional[int] = None, st=None):
        """rows row0 .. row0+B-1: `logits` row r (stride elements apart), token tokens[r], draw counter rng_state[r][1]; `active`:
        the address of the slot engine's active word — row r is predicated on its bit row0 + r"""
        n = self.top_n
        rc = self.L.teal_token_logprobs(logits.data_ptr(), stride, vocab, code, B, tokens.data_ptr(), rng_state.data_ptr(),
                                        self.lp[row0].data_ptr(), self.length, n, self.top_ids[row0].data_ptr() if n else None,
                                        self.top_lp[row0].data_ptr() if n else None, active, row0,
                                        runtime.stream_ptr() if st is None else st)
        if rc != 0:
            _lib.check(rc, "teal_token_logprobs")

    def read(self, row, start: int, n: int):
        """(lp, top_ids, top_lp) of entries start .. start+n-1 of `row` (an index or a slice), cloned"""
        s = slice(start, start + n)
        return self.lp[row, s].clone(), self.top_ids[row, s].clone(), self.top_lp[row, s].clone()
