"""What the fused engines share on the host side: the model's linears and the pointers a captured pass holds, the checks
every dense-chain engine starts `supports` with, and the sampler-side features (token logprobs, logit processors, constraints,
per-request sampling, forced tokens) of the decode engines with the one launch sequence that draws a token under them.  A new per-request feature of the
sampler goes into `SamplerFeatures` only.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..monkeypatch import UP_SHIFT_BYTES, to_column_major
from . import constraints as CN
from . import forcing as FT
from . import logit_processors as PR
from . import logprobs as LP
from . import sampling as SM


def block_linears(layer):
    """the five projections of a block, in launch order"""
    return (layer.attention.wqkv, layer.attention.wo, layer.feed_forward.w1, layer.feed_forward.w3, layer.feed_forward.w2)


def model_linears(model):
    """every block's projections, then the lm_head"""
    return [lin for layer in model.layers for lin in block_linears(layer)] + [model.output]


def relayout(model) -> None:
    """every projection and the lm_head column-major, the decode step's layout (idempotent)"""
    for layer in model.layers:
        for lin in block_linears(layer):
            if not hasattr(lin, "scales_and_zeros"):  # (an int4 image is packed column-gathered already)
                to_column_major(lin, shift_bytes=UP_SHIFT_BYTES if lin is layer.feed_forward.w3 else 0)
    to_column_major(model.output)


def pointer_key(model, weights: bool = True, freqs: bool = True):
    """everything a captured pass over `model` holds raw pointers to: a re-laid-out weight (to_column_major replaces the storage)
    or a re-allocated KV cache changes it.  weights=False: the context length and the KV caches only."""
    head = (model.max_seq_length,)
    if weights:
        head += (model.output.weight.data_ptr(), model.tok_embeddings.weight.data_ptr())
        if freqs:
            head += (model.freqs_cis.data_ptr(),)
    per_layer = []
    for layer in model.layers:
        at, ff = layer.attention, layer.feed_forward
        per_layer += [at.kv_cache.k_cache.data_ptr(), at.kv_cache.v_cache.data_ptr()]
        if weights:
            per_layer += [lin.weight.data_ptr() for lin in (at.wqkv, at.wo, ff.w1, ff.w2, ff.w3)]
    return head + tuple(per_layer)


def dense_16bit_refusal(model, quantised, quantised_why: str) -> Optional[str]:
    """why a dense-chain engine (prompt pass, batched step) cannot take `model`'s weights as they stand, or None: `quantised(lin)`
    marks a quantised linear (refused with `quantised_why`); the rest must be uniformly fp16 / bf16 and on the device"""
    lins = model_linears(model)
    if any(quantised(lin) for lin in lins):
        return quantised_why
    dt = model.output.weight.dtype
    if dt not in (torch.float16, torch.bfloat16) or any(lin.weight.dtype != dt for lin in lins):
        return f"weights are not uniformly fp16 / bf16: {dt}"
    if not model.output.weight.is_cuda:
        return "model is not on a HIP device"
    return None


def slab_chain_refusal(model, shape_why: str, caches_why: str, own_shape: bool = False, then: Optional[str] = None,
                       cache_rule=None) -> Optional[str]:
    """why the dense slab chain (prompt pass, verify pass, batched step) cannot take `model`'s shapes and caches, or None, tried in
    this order: the shape contract (head_dim 64 / 128, dim = n_head * head_dim <= 16384, widths % 256) or the caller's `own_shape`
    -> shape_why; `then`, a reason of the caller's own; freqs_cis in the model dtype; per layer a contiguous KV cache -> caches_why,
    then cache_rule(kv_cache), the caller's own rule (a reason or None)."""
    cfg = model.config
    inter = model.layers[0].feed_forward.w1.out_features
    qd, kv = cfg.n_head * cfg.head_dim, cfg.n_local_heads * cfg.head_dim
    if (cfg.head_dim not in (64, 128) or cfg.dim != qd or cfg.dim % 256 or cfg.dim > 16384 or inter % 256 or (qd + 2 * kv) % 256
            or own_shape):
        return shape_why
    if then is not None:
        return then
    if model.freqs_cis is None or model.freqs_cis.dtype != model.output.weight.dtype:
        return "caches are not set up (model.setup_caches) in the model dtype"
    for layer in model.layers:
        kc = getattr(layer.attention, "kv_cache", None)
        if kc is None or not kc.k_cache.is_contiguous() or not kc.v_cache.is_contiguous():
            return caches_why
        why = cache_rule(kc) if cache_rule is not None else None
        if why is not None:
            return why
    return None


KV_CACHE_FORMATS = (None, "fp8")  # SlotDecodeEngine(kv_cache=): the model's 16-bit caches, or e4m3 rows with power-of-two scales


def kv_cache_refusal(kind: str, kv_cache: Optional[str]) -> Optional[str]:
    """why the `kind` engine ("slot", "batched", "decode", "speculative", "tensor-parallel") cannot take kv_cache=, or None.  The fp8
    cache is filled where a request is admitted: rows leave the 16-bit prompt pass through teal_kv8_quantize_rows, so only the
    engine that admits can hold one."""
    if kv_cache is None:
        return None
    if kv_cache not in KV_CACHE_FORMATS:
        return f"unknown kv_cache {kv_cache!r} (None: the model's 16-bit caches; 'fp8': e4m3 rows with power-of-two scales)"
    if kind != "slot":
        return (f"kv_cache={kv_cache!r} is SlotDecodeEngine's (continuous batching): the {kind} path has no admission to quantise "
                "a prompt's rows at")
    return None


class _SlotCaches:
    """the K / V base pointers of slot `slot` of batch-B caches: slot s of a contiguous [B, n_kv, max_seq, hd] cache is itself a
    contiguous [1, n_kv, max_seq, hd] cache"""

    slot = 0

    def _caches(self, at):
        kc, vc = at.kv_cache.k_cache, at.kv_cache.v_cache
        off = self.slot * kc[0].numel() * kc.element_size()
        return kc.data_ptr() + off, vc.data_ptr() + off


class SamplerFeatures:
    """Token logprobs (logprobs.py: one launch behind the sampler), per-request logit processors (logit_processors.py: one
    launch in front of it), constraints (constraints.py: one launch between the two, on a slot engine) and per-request sampling
    (sampling.py: one launch in the samplers' place) and forced tokens (forcing.py: one launch behind the samplers, on a slot
    engine), all off until switched on,
    and `_draw`, the launches of a draw under them.  The host class provides `_feature_rows` (its sequences), `history` (int32
    [..., length]: a logprob row is as long), `cfg.vocab_size`, `dtype`, `code`, a `_graph` the setters drop and `_sample_row`."""

    _lp: Optional[LP.LogprobBuffers] = None      # set_logprobs
    _proc: Optional[PR.LogitProcessors] = None   # set_logit_processors
    _samp: Optional[SM.SamplingParams] = None    # set_sampling_params
    _con: Optional[CN.Constraints] = None        # set_constraints (a slot engine's)
    _frc: Optional[FT.ForcedTokens] = None       # set_forced_tokens (a slot engine's)
    _active: Optional[int] = None                # the address of a slot engine's active word: its launches are predicated on it

    def _feature_refusal(self, what: str) -> None:
        """raises if this engine cannot switch `what` ("logprobs" / "logit processors" / "per-request sampling") on"""
        return None

    def set_logprobs(self, n: Optional[int]):
        """None: off (the default; the step's launches are exactly those without this feature).  0: every token the fused sampler
        draws gets its logprob under the model's own distribution (temperature 1, no top-k filter); 1..8: and the ids and logprobs
        of that many most likely tokens.  Entry i of a sequence belongs to entry i of its history row (read_logprobs).  Drops the
        captured graphs."""
        n = LP.check_setting(n)
        if n is not None:
            self._feature_refusal("logprobs")
        self._lp = None if n is None else LP.LogprobBuffers(self._feature_rows, self.history.shape[-1], n, self.history.device)
        self._graph = None

    def _logprobs(self) -> LP.LogprobBuffers:
        if self._lp is None:
            raise RuntimeError("logprobs are off (set_logprobs)")
        return self._lp

    def set_logit_processors(self, on: bool):
        """off (the default): the step's launches are exactly those without this feature.  on: the fused sampler draws from the
        step's logits adjusted by each sequence's repetition / presence / frequency penalty and logit bias (set_slot_processors;
        identity until set), kept in a buffer of their own; logprobs and `logits` stay the model's.  Drops the captured graphs."""
        if on:
            self._feature_refusal("logit processors")
        self._proc = PR.LogitProcessors(self._feature_rows, self.cfg.vocab_size, self.dtype, self.history.device) if on else None
        self._graph = None

    def _processors(self) -> PR.LogitProcessors:
        if self._proc is None:
            raise RuntimeError("logit processors are off (set_logit_processors)")
        return self._proc

    def set_slot_processors(self, slot: int, prompt_tokens, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                            frequency_penalty: float = 0.0, logit_bias: Optional[Dict] = None):
        """sequence `slot` starts over: nothing generated yet, `prompt_tokens` marked as its prompt, and these controls from its
        next draw on.  ValueError with the reason: repetition_penalty not finite and > 0, a penalty not finite, a bias id outside
        the vocabulary or a bias value not finite."""
        self._processors().set_row(slot, prompt_tokens, repetition_penalty, presence_penalty, frequency_penalty, logit_bias)

    def set_sampling_params(self, on: bool):
        """off (the default): the step's launches are exactly those without this feature, one fused top-k sampler per sequence
        under the temperature and top_k the step is given.  on: ONE launch draws every sequence's token under that sequence's own
        temperature, top_k, top_p and min_p (set_slot_sampling; temperature 1 and no filter until set), read from device memory:
        the step no longer depends on the temperature and top_k it is given, and one captured step serves any mix.  Drops the
        captured graphs."""
        if on:
            self._feature_refusal("per-request sampling")
        self._samp = SM.SamplingParams(self._feature_rows, self.cfg.vocab_size, self.dtype, self.history.device) if on else None
        self._graph = None

    def _sampling(self) -> SM.SamplingParams:
        if self._samp is None:
            raise RuntimeError("per-request sampling is off (set_sampling_params)")
        return self._samp

    def set_slot_sampling(self, slot: int, temperature: float, top_k: Optional[int], top_p: float = 1.0, min_p: float = 0.0):
        """sequence `slot` draws under these settings from its next draw on.  ValueError with the reason: a setting not finite,
        temperature < 0, top_k negative, top_p <= 0, min_p outside [0, 1)."""
        self._sampling().set_row(slot, temperature, top_k, top_p, min_p)

    # the sampling rows (None while the feature is off): the parameter words and each row's last kept count
    sampling_params = property(lambda self: None if self._samp is None else self._samp.params)
    sampling_kept = property(lambda self: None if self._samp is None else self._samp.kept)

    def set_constraints(self, on: bool, capacity_words: int = 1 << 20):
        """constrained decoding belongs to the slot engine: an automaton starts over at an admission and opens the request's EOS id,
        and this engine has neither — switching it on is refused with that reason (off is what it is)"""
        if on:
            raise NotImplementedError(f"{type(self).__name__} has no constrained decoding: a constraint starts at an admission and ends on "
                                      "the request's EOS word, which only SlotDecodeEngine has")

    def set_slot_sparsity(self, on: bool):
        """per-request sparsity belongs to the slot engine: a request's thresholds are written at its admission, and this engine
        has none — switching it on is refused with that reason (off is what it is)"""
        if on:
            raise NotImplementedError(f"{type(self).__name__} has no per-request sparsity: a request's thresholds are written at its "
                                      "admission, which only SlotDecodeEngine has")

    def set_forced_tokens(self, on: bool, capacity: Optional[int] = None):
        """forced tokens belong to the slot engine: a request's tokens are written at its admission, and this engine has none —
        switching them on is refused with that reason (off is what it is)"""
        if on:
            raise NotImplementedError(f"{type(self).__name__} has no forced tokens: a request's tokens are written at its admission, and "
                                      "this engine has no admission (only SlotDecodeEngine has)")

    def _forced(self) -> FT.ForcedTokens:
        if self._frc is None:
            raise RuntimeError("forced tokens are off (set_forced_tokens)")
        return self._frc

    def _constraints(self) -> CN.Constraints:
        if self._con is None:
            raise RuntimeError("constraints are off (set_constraints)")
        return self._con

    def _eos_words(self, row0: int) -> int:
        """the address of sequence row0's EOS word (int32, one per sequence): the constrain launch's `eos`"""
        raise NotImplementedError

    def _step_key(self, temperature, top_k):
        """the sampler's share of a captured step's key: the two scalars baked into the fused top-k sampler's launches, or —
        per-request sampling on — nothing, the rows being read on the device"""
        return (float(temperature), int(top_k or 0)) if self._samp is None else ("rows",)

    # the processors' buffers (None while they are off): what the samplers read, the state table, the parameter and bias rows
    adj_logits = property(lambda self: None if self._proc is None else self._proc.adj)
    lp_state = property(lambda self: None if self._proc is None else self._proc.state)
    lp_params = property(lambda self: None if self._proc is None else self._proc.params)
    lp_bias = property(lambda self: None if self._proc is None else self._proc.bias)

    def _sample_row(self, row: int, logits: torch.Tensor, temperature, top_k, feed: bool, st):
        """the engine's fused top-k sampler, one launch: sequence `row` draws from its row `logits`; feed: the token also moves
        the sequence's position and history on"""
        raise NotImplementedError

    def _draw(self, logits: torch.Tensor, stride: int, rows: int, temperature, top_k, rng_state: torch.Tensor, tokens: torch.Tensor,
              pos: Optional[torch.Tensor], history: Optional[torch.Tensor], count_token: bool, row0: int = 0,
              fed: Optional[torch.Tensor] = None, st=None):
        """Sequences row0 .. row0+rows-1 draw their next token from `logits` (rows `stride` elements apart; 0: the one row as it
        stands): the processors' launch (if on), the constrain launch (if on) over what they left, then ONE sampling launch over the rows or the fused top-k sampler row by row,
        then the forcing launch (if on), which puts a row's forced token in the drawn one's place, then the logprob launch (if on)
        over the logits as the model gave them.  rng_state / tokens / pos / history are the first
        row's; pos and history None: the draw feeds no loop state.  count_token: the processors first count each row's token in
        `fed` (default `tokens`: the buffer the step was fed from) as generated."""
        active, src = self._active, logits
        if self._proc is not None:
            self._proc.launch(logits, stride, rows, tokens if fed is None else fed, count_token, row0=row0, active=active, st=st)
            src = self._proc.adj[row0:row0 + rows] if stride else self._proc.adj[row0]
        if self._con is not None:  # each row's automaton moves on the token it was fed, then masks the row the samplers read
            self._con.launch(src, stride, rows, tokens if fed is None else fed, rng_state, self._eos_words(row0), row0=row0, active=active,
                             st=st)
            src = self._con.con[row0:row0 + rows] if stride else self._con.con[row0]
        if self._samp is not None:  # one launch, every row under its own settings
            self._samp.launch(src, stride, rows, rng_state, tokens, pos, history, self.history.shape[-1], row0=row0, active=active, st=st)
        else:
            for r in range(rows):
                self._sample_row(row0 + r, src[r] if stride else src, temperature, top_k, pos is not None, st)
        if self._frc is not None:  # behind the samplers, in front of everything that reads the drawn token
            self._frc.launch(rows, rng_state, tokens, history, self.history.shape[-1], row0=row0, active=active, st=st)
        if self._lp is not None:  # (a slot engine: predicated on the active word the samplers saw — retire clears bits behind it)
            self._lp.launch(logits, stride, self.cfg.vocab_size, self.code, rows, tokens, rng_state, row0=row0, active=active, st=st)

    def _feature_loop_state(self):
        """the features' share of what a captured step carries from replay to replay"""
        return (list(self._lp.tensors()) if self._lp is not None else []) + \
               (list(self._proc.loop_tensors()) if self._proc is not None else []) + \
               (list(self._samp.loop_tensors()) if self._samp is not None else []) + \
               (list(self._con.loop_tensors()) if self._con is not None else [])

    def _feature_key(self):
        """the features' share of a captured step's key (per-request sampling, constraints and forced tokens add their word only
        while on)"""
        return (None if self._lp is None else self._lp.top_n, self._proc is not None) + (("sampling",) if self._samp is not None else ()) + \
               (("constraints",) if self._con is not None else ()) + (("forced",) if self._frc is not None else ())
