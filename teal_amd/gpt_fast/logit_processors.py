"""Per-request logit processors of the fused engines (teal_amd/csrc/teal_logit_adjust.hip): the buffers an engine keeps per slot
and the one launch that turns a step's logits into the row its sampler reads.

Order of application, per vocabulary entry: repetition penalty (on every token of the prompt — a shared prefix included — and
every generated token: a positive logit is divided by it, any other multiplied), frequency penalty (times the number of times
the token was generated), presence penalty (once, if it was generated at all), logit bias; the result is clamped to the dtype's
finite range.  The launch reads its parameters and its counts from device memory and is predicated per slot, so an admission
changes them without re-capturing the step, and it counts the token the step was fed — the request's most recently generated
one — itself.  The step's own logits stay as the model left them: logprobs, admit_logits and dumps read those.
"""
from __future__ import annotations

import math
import struct
from typing import Dict, Optional, Sequence

import torch

from .. import _lib, runtime

PROMPT_BIT = -2 ** 31  # bit 31 of a state word: the token occurs in the request's prompt


def fp32(v) -> float:
    """v rounded to fp32 (+-inf where it overflows)"""
    try:
        return struct.unpack("f", struct.pack("f", float(v)))[0]
    except OverflowError:
        return math.copysign(math.inf, float(v))


MAX_VOCAB = 131072  # teal_logit_adjust: vocab a multiple of 8 in 8 .. 131072


def check_controls(vocab: Optional[int], repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None) -> Dict:
    """the four controls, validated (ValueError with the reason) and normalised: floats and {int id: float value} or None.
    vocab None: the ids' upper bound is not checked (before a model is known)."""
    def real(name, v):
        # judged as the fp32 value the parameter row will hold: 1e39 is finite as a double and +inf there, 1e-50 is 0
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not math.isfinite(fp32(v)):
            raise ValueError(f"{name} must be a finite number (in fp32), got {v!r}")
        return float(v)
    theta = real("repetition_penalty", repetition_penalty)
    if fp32(theta) <= 0.0:
        raise ValueError(f"repetition_penalty must be > 0 in fp32 (1: off), got {repetition_penalty!r}")
    bias = None
    if logit_bias is not None:
        if not isinstance(logit_bias, dict):
            raise ValueError(f"logit_bias must map token ids to values, got {type(logit_bias).__name__}")
        bias = {}
        for k, v in logit_bias.items():
            try:
                if isinstance(k, bool) or isinstance(k, float):
                    raise ValueError
                t = int(k)
            except (TypeError, ValueError):
                raise ValueError(f"logit_bias: {k!r} is not a token id") from None
            if t < 0 or (vocab is not None and t >= vocab):
                raise ValueError(f"logit_bias: token id {t} outside 0..{vocab - 1 if vocab is not None else 'vocab-1'}")
            bias[t] = real(f"logit_bias[{t}]", v)
    return {"repetition_penalty": theta, "presence_penalty": real("presence_penalty", presence_penalty),
            "frequency_penalty": real("frequency_penalty", frequency_penalty), "logit_bias": bias or None}


def is_identity(c: Dict) -> bool:
    """no control of `c` (a dict of the four, or a subset) changes a logit"""
    return (c.get("repetition_penalty", 1.0) == 1.0 and c.get("presence_penalty", 0.0) == 0.0
            and c.get("frequency_penalty", 0.0) == 0.0 and not c.get("logit_bias"))


class LogitProcessors:
    """adj [rows][vocab] (what the samplers read), state int32 [rows][vocab] (bit 31: prompt token; low bits: times generated),
    params fp32 [rows][4] = {theta, alpha_p, alpha_f, reserved}, bias [rows][vocab] — on `device`, rows = the engine's slots"""

    def __init__(self, rows: int, vocab: int, dtype: torch.dtype, device):
        if vocab < 8 or vocab > MAX_VOCAB or vocab % 8:  # (refused here, not by the first launch in the middle of an admission)
            raise ValueError(f"logit processors need a vocabulary that is a multiple of 8 in 8..{MAX_VOCAB} (the processor launch's "
                             f"contract), got {vocab}")
        self.rows, self.vocab, self.dtype = int(rows), int(vocab), dtype
        self.adj = torch.zeros(rows, vocab, dtype=dtype, device=device)
        self.state = torch.zeros(rows, vocab, dtype=torch.int32, device=device)
        self.params = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * rows, dtype=torch.float32, device=device)
        self.bias = torch.zeros(rows, vocab, dtype=dtype, device=device)
        self.code = runtime.dtype_code(dtype)
        self.L = _lib.load()

    def loop_tensors(self):
        """what a captured step changes from replay to replay"""
        return (self.state,)

    def _tokens(self, toks, what: str) -> torch.Tensor:
        t = torch.as_tensor(toks, dtype=torch.int64).view(-1)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.vocab):
            raise ValueError(f"{what}: token ids must be in 0..{self.vocab - 1}")
        return t.to(self.state.device)

    def reset(self, row: int, prompt_tokens: Sequence[int]):
        """row's state: nothing generated yet, bit 31 on the prompt's tokens (plain indexing: outside capture)"""
        t = self._tokens(prompt_tokens, "prompt_tokens")
        self.state[row].zero_()
        if t.numel():
            self.state[row].index_fill_(0, t, PROMPT_BIT)

    def set_row(self, row: int, prompt_tokens: Sequence[int], repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                frequency_penalty: float = 0.0, logit_bias: Optional[Dict] = None):
        if not 0 <= int(row) < self.rows:
            raise ValueError(f"slot {row} outside 0..{self.rows - 1}")
        c = check_controls(self.vocab, repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
        ids = vals = None
        if c["logit_bias"]:
            ids = torch.tensor(list(c["logit_bias"].keys()), dtype=torch.int64)
            vals = torch.tensor(list(c["logit_bias"].values()), dtype=torch.float32).to(self.dtype)
            if not bool(torch.isfinite(vals).all()):
                raise ValueError(f"logit_bias: a value is not finite in {self.dtype}")
        self.reset(row, prompt_tokens)
        self.params[row].copy_(torch.tensor([c["repetition_penalty"], c["presence_penalty"], c["frequency_penalty"], 0.0]))
        self.bias[row].zero_()
        if ids is not None:
            self.bias[row].index_copy_(0, ids.to(self.bias.device), vals.to(self.bias.device))

    def launch(self, logits: torch.Tensor, stride: int, B: int, tokens: torch.Tensor, count_token: bool, row0: int = 0,
               active: Optional[int] = None, st=None):
        """rows row0 .. row0+B-1: `logits` row r (stride elements apart) -> adj[row0 + r]; count_token: tokens[r] is counted as
        generated first; `active`: the address of the slot engine's active word — row r is predicated on its bit row0 + r"""
        rc = self.L.teal_logit_adjust(logits.data_ptr(), stride, self.vocab, self.code, B, tokens.data_ptr(), int(bool(count_token)),
                                      self.state[row0].data_ptr(), self.params[row0].data_ptr(), self.bias[row0].data_ptr(),
                                      self.adj[row0].data_ptr(), self.vocab, active, row0, runtime.stream_ptr() if st is None else st)
        if rc != 0:
            _lib.check(rc, "teal_logit_adjust")
