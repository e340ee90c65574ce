"""Speculative decoding (gpt-fast/generate.py:98-217): a TEAL-sparse draft proposes k tokens, the DENSE model verifies them in one
pass, and the reference's accept / reject rule keeps the dense model's output distribution.

One round, k + 1 .. k + 2 launches' worth of work per draft token and nothing on the host in between:

    k draft steps      DecodeEngine (the fused sparse step), each recording its logits row into dlog[j] and drawing d_{j+1}
                       with the fused sampler into tokens[j + 1]
    [fill-in step]     separate draft model only: the draft's own KV row of d_k (gpt-fast/generate.py:131-136), run every round
    verify             VerifyPass: the prompt pass's launches over [x0, d1 .. dk] at positions p .. p+k (p on the device), with
                       teal_verify_attention against the whole cache and the lm_head of EVERY row (teal_prefill_gemm)
    accept             teal_spec_accept: accepted count, emitted tokens appended to a device sequence, the next round's position
                       and input token, a histogram of accepted counts

Self-speculation: the draft is the target's own weights with TEAL thresholds — one weight copy, one KV cache; the verify pass
rewrites rows p .. p+k with dense K / V, so no fill-in is needed.  A separate draft model has its own engine and caches.
`SpeculativeDecoder.round()` replays one hipGraph per round (`graph=True`) or issues the same launches eagerly.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import _lib, runtime
from .engine import DecodeEngine
from .engine_features import kv_cache_refusal
from .model import Transformer
from .prefill import MAX_T, PrefillEngine

MAX_K = MAX_T - 1  # T = k + 1 verified rows per pass


class VerifyPass(PrefillEngine):
    """The dense pass over T <= 16 tokens at positions p .. p+T-1, p read from a device int32: every layer's K / V rows p .. p+T-1
    are written and the lm_head slabs of all T rows are left in `lm_slabs` (teal_spec_accept sums and rounds them)."""

    @staticmethod
    def supports(model: Transformer) -> Optional[str]:
        """None if the verify pass can run `model`, else the reason (there is no module-path verify)."""
        why = PrefillEngine.supports(model)
        if why is not None:
            return why
        if model.config.vocab_size % 256:
            return f"vocab_size {model.config.vocab_size} is not a multiple of 256 (the all-row lm_head GEMM's column contract)"
        return None

    def __init__(self, model: Transformer):
        why = type(self).supports(model)
        if why is not None:
            raise ValueError(f"speculative decoding cannot verify with this model: {why}")
        super().__init__(model)
        cfg, dev = model.config, model.output.weight.device
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        smax = max(1, min(ncu // (cfg.vocab_size // 256), self.dim // 256, 16))  # teal_prefill_gemm's largest split for the lm_head
        self.lm_slabs = torch.zeros(smax * cfg.vocab_size * MAX_T, device=dev, dtype=torch.float32)
        nb = int(self.L.teal_verify_attention_ws_bytes(MAX_T, cfg.n_head, cfg.head_dim))
        self.partials = torch.zeros((nb + 3) // 4, device=dev, dtype=torch.float32)

    def run(self, tokens: torch.Tensor, pos: torch.Tensor, T: int) -> int:
        """tokens: int32 [>= T] on the device, pos: int32 [1] on the device (the first token's position).  Returns the lm_head's
        split (slices of `lm_slabs` to sum)."""
        assert 1 <= T <= MAX_T and tokens.dtype == torch.int32 and pos.dtype == torch.int32
        m, cfg, L, st = self.model, self.model.config, self.L, runtime.stream_ptr()

        def attention(at, A, ns):
            kc, vc = self._caches(at)
            rc = L.teal_verify_attention(A.data_ptr(), ns, self.rope.data_ptr(), pos.data_ptr(), kc, vc, self.yt.data_ptr(),
                                         self.partials.data_ptr(), self.partials.numel() * 4, T, cfg.n_head, cfg.n_local_heads, cfg.head_dim,
                                         self.max_seq, self.code, st)
            if rc != 0:
                _lib.check(rc, "teal_verify_attention")

        self._dense_walk(T, tokens.data_ptr(), attention, st)
        return self._gemm(self._norm_in(m.norm.weight), m.output, None, self.dim, T, self.lm_slabs, st)

    @torch.no_grad()
    def all_logits(self, tokens: torch.Tensor, pos: int) -> torch.Tensor:
        """[T, vocab] logits of tokens at positions pos .. pos+T-1 (tests: the slabs summed in slice order, rounded once)."""
        T, V = int(tokens.numel()), self.model.config.vocab_size
        dev = self.lm_slabs.device
        ns = self.run(tokens.to(torch.int32).contiguous(), torch.tensor([pos], dtype=torch.int32, device=dev), T)
        kr = 8 if T <= 8 else 16
        s = self.lm_slabs[:ns * V * kr].view(ns, V, kr)
        acc = s[0].clone()
        for i in range(1, ns):
            acc += s[i]
        return acc[:, :T].t().to(self.model.output.weight.dtype)


class SpeculativeDecoder:
    """Rounds of k draft steps + verify + accept.  `draft`: the DecodeEngine that proposes (its rng_state and position buffer are
    the round's); `verify`: the target's VerifyPass.  `fill_in`: the draft has KV caches of its own (a separate draft model)."""

    def __init__(self, draft: DecodeEngine, verify: VerifyPass, k: int, temperature: float, top_k: Optional[int], fill_in: bool,
                 capacity: int, graph: bool = True, kv_cache: Optional[str] = None):
        why = kv_cache_refusal("speculative", kv_cache)
        if why is not None:
            raise ValueError(f"speculative decoding: {why}")
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"speculative decoding: speculate_k must be in 1..{MAX_K}, got {k}")
        V = verify.model.config.vocab_size
        if draft.cfg.vocab_size != V or draft.dtype != verify.model.output.weight.dtype:
            raise ValueError("speculative decoding: the draft and the target must share the vocabulary and the 16-bit dtype")
        if draft.sampling_params is not None:
            raise ValueError("speculative decoding: the draft engine has per-request sampling on (set_sampling_params(False) first)")
        draft.speculating = True  # per-request sampling stays off on this engine (DecodeEngine._feature_refusal) until release()
        self.draft, self.verify, self.k, self.fill_in, self.graph = draft, verify, int(k), bool(fill_in), bool(graph)
        self.temperature, self.top_k = float(temperature), int(top_k or 0)
        self.L = draft.L
        dev = draft.logits.device
        i32 = dict(device=dev, dtype=torch.int32)
        self.tokens = torch.zeros(MAX_T, **i32)         # [x0, d1 .. dk]
        self.spec_pos = torch.zeros(1, **i32)           # the round's base position p (the position of x0)
        self.dlog = torch.zeros(self.k, V, device=dev, dtype=draft.dtype)
        self.fill_logits = torch.zeros(1, 1, V, device=dev, dtype=draft.dtype)
        self.capacity = int(capacity)
        self.out_seq = torch.zeros(max(1, self.capacity), **i32)
        self.out_len = torch.zeros(1, **i32)
        self.n_acc = torch.zeros(1, **i32)
        self.hist = torch.zeros(MAX_T, **i32)
        nb = int(self.L.teal_spec_accept_scratch_bytes(V, self.k))
        self.scratch = torch.zeros((nb + 3) // 4, device=dev, dtype=torch.float32)
        self._graph = None

    def release(self):
        """the decoder lets its draft engine go: the engine may switch per-request sampling on again.  The decoder must not run
        another round afterwards."""
        self.draft.speculating = False
        self._graph = None

    def begin(self, first_token: torch.Tensor, pos: int):
        """the next round drafts from `first_token` at position `pos`; the emitted sequence and the histogram restart"""
        self.tokens[0:1].copy_(first_token.view(1).to(torch.int32))
        self.spec_pos.fill_(int(pos))
        self.draft.pos_buf.fill_(int(pos))
        self.out_len.zero_()
        self.hist.zero_()

    def _launch_round(self):
        eng, k, V = self.draft, self.k, self.verify.model.config.vocab_size
        st = runtime.stream_ptr()
        for j in range(k):
            eng(self.tokens[j:j + 1].view(1, 1), eng.pos_buf, logits_out=self.dlog[j])
            rc = self.L.teal_sample_topk_ws(self.dlog[j].data_ptr(), V, eng.code, self.top_k, self.temperature, eng.rng_state.data_ptr(),
                                            self.tokens[j + 1:].data_ptr(), eng.pos_buf.data_ptr(), None, 0, eng.ws.data_ptr(),
                                            eng.ws.numel() * 4, st)
            if rc != 0:
                _lib.check(rc, "teal_sample_topk (draft)")
        if self.fill_in:  # the draft's own KV row of d_k at p + k (used when all k are accepted; rewritten otherwise)
            eng(self.tokens[k:k + 1].view(1, 1), eng.pos_buf, logits_out=self.fill_logits)
        ns = self.verify.run(self.tokens, self.spec_pos, k + 1)
        rc = self.L.teal_spec_accept(self.verify.lm_slabs.data_ptr(), ns, self.dlog.data_ptr(), V, k, eng.code, self.top_k, self.temperature,
                                     eng.rng_state.data_ptr(), self.tokens.data_ptr(), self.spec_pos.data_ptr(), eng.pos_buf.data_ptr(),
                                     self.out_seq.data_ptr(), self.capacity, self.out_len.data_ptr(), self.n_acc.data_ptr(),
                                     self.hist.data_ptr(), self.scratch.data_ptr(), self.scratch.numel() * 4, st)
        if rc != 0:
            _lib.check(rc, "teal_spec_accept")

    def capture(self):
        """one hipGraph of a whole round (warm-up outside capture; the state it advanced is put back)"""
        if self._graph is None:
            e = self.draft
            self._graph, _ = runtime.capture_graph(self._launch_round, (self.tokens, self.spec_pos, e.pos_buf, e.rng_state, self.out_len,
                                                                        self.n_acc, self.hist, self.out_seq))
        return self._graph

    @torch.no_grad()
    def round(self) -> int:
        """one round; returns the accepted count (the round's one host synchronisation)"""
        if self.graph:
            self.capture().replay()
        else:
            self._launch_round()
        return int(self.n_acc.item())

    @torch.no_grad()
    def decode(self, first_token: torch.Tensor, pos: int, n: int) -> torch.Tensor:
        """at least n tokens after `first_token` (at `pos`); returns exactly n of them"""
        self.begin(first_token, pos)
        if self.graph:
            self.capture()  # (its warm-up round runs at this position and puts the state back: the real round rewrites the same rows)
        emitted = 0
        while emitted < n:
            emitted += self.round() + 1
        return self.out_seq[:n].clone()

    def histogram(self) -> List[int]:
        """rounds per accepted count 0 .. k since begin()"""
        return [int(x) for x in self.hist[:self.k + 1].tolist()]

    @staticmethod
    def acceptance_stats(hist: List[int]) -> Dict[str, object]:
        """the reference's printout (gpt-fast/generate.py:517-520): fraction of rounds per accepted count, mean accepted"""
        tot = max(1, sum(hist))
        probs = [h / tot for h in hist]
        return {"acceptance_probs": probs, "mean_accepted": sum(i * p for i, p in enumerate(probs))}
