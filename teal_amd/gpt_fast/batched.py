"""Batched decode: one fused step for B <= 8 TEAL-sparse sequences (teal_amd/csrc/teal_batched.hip).

TEAL's rule is per token (the reference's SparsifyFn masks every token's activations against the site's threshold), so
sequence b's projection is W . (x_b * [|x_b| > tau]).  A step streams every weight row that ANY sequence keeps — the union —
once, and each sequence adds only its own kept rows.  With independent activations at 50 % kept per sequence the union holds
about 1 - 0.5^B of the rows, so the bytes per step grow with B while the tokens per step grow as B.

One layer, the prompt pass's hand-over layout [feature][8] (slot b = sequence b):

    gemm(wqkv, tau_q | tau_k | tau_v) [RMSNorm while staging] -> attention (RoPE at pos[b], row pos[b] of cache b, split-KV)
    -> gemm(wo, tau_o) -> resid -> gemm(w1 | w3, tau_gate | tau_up) [RMSNorm while staging]
    -> gemm(w2, tau_down) [silu * up while staging] -> resid
                                 ... -> gemm(lm_head, tau = -inf) [final RMSNorm while staging] -> logits [B, vocab]

The embedding rows of the B current tokens enter through teal_prefill_resid_norm.  Sampling is B launches of the fused sampler,
each with its own rng_state / token / position / history, so one hipGraph replay is one step for all B sequences.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional

import torch

from .. import _lib, runtime
from ..kernels.sparse_gemv import BATCH_MAX, batched_segs
from . import constraints as CN
from . import forcing as FT
from . import logit_processors as PR
from . import sampling as SM
from . import stopping as ST
from .engine_features import SamplerFeatures, _SlotCaches, dense_16bit_refusal, kv_cache_refusal, slab_chain_refusal
from .model import Transformer
from .prefill import MAX_T, PrefillEngine, PrefillIn, SlabChain
from .speculative import VerifyPass

PROJ_LAUNCHES = (("qkv", ("q", "k", "v")), ("o", ("o",)), ("gateup", ("gate", "up")), ("down", ("down",)))
PROJ_KEYS = tuple(p for _, projs in PROJ_LAUNCHES for p in projs)  # the keys of one layer's thresholds dict
NINF = float("-inf")


class BatchedDecodeEngine(SlabChain, SamplerFeatures):
    _kv_kind = "batched"  # kv_cache_refusal's name of this engine

    @staticmethod
    def supports(model: Transformer, kv_cache: Optional[str] = None) -> Optional[str]:
        """None if the batched step can run `model` as it stands (batch = the caches' max_batch_size), else the reason."""
        why = kv_cache_refusal("batched", kv_cache)
        if why is not None:
            return why
        cfg = model.config
        if int(getattr(model, "tp_world", 1)) > 1:
            return "tensor-parallel models are not batched (decode them one sequence at a time)"
        why = dense_16bit_refusal(
            model, lambda lin: hasattr(lin, "scales_and_zeros") or hasattr(lin, "scales") or lin.weight.dtype == torch.int8,
            "quantised (int8 / int4) weights are not batched")
        if why is not None:
            return why
        inter = model.layers[0].feed_forward.w1.out_features
        kv = cfg.n_local_heads * cfg.head_dim
        caches_why = "KV caches must be contiguous [B, n_kv, max_seq, head_dim] tensors"
        sizes = []  # the layers' batch sizes

        def one_batch_size(kc):
            if kc.k_cache.dim() != 4:
                return caches_why
            sizes.append(kc.k_cache.shape[0])
            if kc.k_cache.shape[0] != sizes[0] or kc.v_cache.shape[0] != sizes[0]:
                return "KV caches must share one batch size"
            return None

        why = slab_chain_refusal(model, "shape outside the batched kernels' contract (head_dim 64 / 128, dim = n_head * head_dim <= 16384, "
                                 "dim / intermediate / qkv width / vocab multiples of 256)", caches_why,
                                 own_shape=bool(inter > 65536 or kv % 8 or cfg.vocab_size % 256), cache_rule=one_batch_size)
        if why is not None:
            return why
        B = sizes[0] if sizes else None
        if B is None or not 1 <= B <= BATCH_MAX:
            return f"batch size {B} outside 1..{BATCH_MAX} (setup_caches(max_batch_size=B))"
        return None

    def __init__(self, model: Transformer, thresholds: List[Dict[str, float]], batch: int, kv_cache: Optional[str] = None):
        why = kv_cache_refusal(self._kv_kind, kv_cache)
        if why is not None:
            raise ValueError(f"{type(self).__name__}: {why}")
        self.kv_cache = kv_cache
        why = BatchedDecodeEngine.supports(model)
        if why is not None:
            raise ValueError(f"BatchedDecodeEngine cannot run this model: {why}")
        B = int(batch)
        cache_b = model.layers[0].attention.kv_cache.k_cache.shape[0]
        if kv_cache is not None and not 1 <= B <= BATCH_MAX:  # (fp8: the slots are the engine's own, not the model's caches)
            raise ValueError(f"{type(self).__name__}: batch {B} outside 1..{BATCH_MAX}")
        if kv_cache is None and (not 1 <= B <= BATCH_MAX or B != cache_b):
            raise ValueError(f"BatchedDecodeEngine: batch {B} must equal the caches' max_batch_size ({cache_b}) and be <= {BATCH_MAX}")
        if len(thresholds) != len(model.layers):
            raise ValueError("one thresholds dict per layer")
        SlabChain.__init__(self, model, BATCH_MAX)
        self.cfg, self.B = model.config, B
        self._feature_rows = B
        cfg = self.cfg
        dev, dt = model.output.weight.device, model.output.weight.dtype
        self.dtype = dt
        self.ths = [dict(t) for t in thresholds]
        V = cfg.vocab_size
        z = lambda *shape, dtype=dt: torch.zeros(*shape, device=dev, dtype=dtype)  # noqa: E731
        i32 = dict(dtype=torch.int32)
        self.tok_buf = z(BATCH_MAX, **i32)   # the B current tokens
        self.pos_buf = z(BATCH_MAX, **i32)   # the B positions (device; may differ)
        self.lm_slabs = z(16 * V * BATCH_MAX, dtype=torch.float32)
        self.logits = z(B, V)
        nb = int(self.L.teal_batched_decode_attention_ws_bytes(B, cfg.n_head, cfg.head_dim))
        self.partials = z((nb + 3) // 4, dtype=torch.float32)
        # kept counts of the last step: [layer][launch][slice 16][segment 3][9] (per sequence, union)
        self.counts = z(len(model.layers), len(PROJ_LAUNCHES), 16 * 3 * 9, **i32)
        self.splits = [[0] * len(PROJ_LAUNCHES) for _ in model.layers]
        # sampling state, one set per sequence
        self.rng_state = torch.zeros(B, 2, dtype=torch.int64, device=dev)
        self.history = z(B, self.max_seq + 1, **i32)
        self._seed = 1234
        self._graph = None
        self._graph_key = None
        kvw = self.kv
        self._segs = [{
            "qkv": batched_segs([self.dim, self.dim + kvw, self.nqkv], [t["q"], t["k"], t["v"]]),
            "o": batched_segs([self.dim], [t["o"]]),
            "gateup": batched_segs([self.inter, 2 * self.inter], [t["gate"], t["up"]]),
            "down": batched_segs([self.dim], [t["down"]]),
        } for t in self.ths]
        self._lm_segs = batched_segs([V], [NINF])

    # ---- launches: with `_active` (SlotDecodeEngine: the address of its active word) the slot-predicated entry points --------
    def _gemm(self, gin: PrefillIn, segs, lin0, lin1, Z: int, out: torch.Tensor, counts: Optional[torch.Tensor], st,
              taus: Optional[int] = None) -> int:
        """taus (a slot engine with per-request sparsity on): the address of the launch's [3][8] threshold table"""
        w0, w1 = lin0.weight, lin1.weight if lin1 is not None else None
        head = (ctypes.byref(gin), ctypes.byref(segs), w0.data_ptr(), w0.stride(1), w0.shape[0], w1.data_ptr() if lin1 is not None else None,
                w1.stride(1) if lin1 is not None else 0, w1.shape[0] if lin1 is not None else 0, out.data_ptr(), out.numel() * 4, Z, self.B)
        tail = (counts.data_ptr() if counts is not None else None, self.code, ctypes.byref(self._split), st)
        if self._active is None:
            rc, what = self.L.teal_batched_sparse_gemm(*head, *tail), "teal_batched_sparse_gemm"
        elif taus is not None:
            rc, what = self.L.teal_batched_sparse_gemm_slot_taus(*head, self._active, taus, *tail), "teal_batched_sparse_gemm_slot_taus"
        else:
            rc, what = self.L.teal_batched_sparse_gemm_slots(*head, self._active, *tail), "teal_batched_sparse_gemm_slots"
        if rc != 0:
            _lib.check(rc, what)
        return self._split.value

    def _attention(self, at, A: torch.Tensor, ns: int, st):
        cfg = self.cfg
        head = (A.data_ptr(), ns, self.rope.data_ptr(), self.pos_buf.data_ptr())
        tail = (at.kv_cache.k_cache.data_ptr(), at.kv_cache.v_cache.data_ptr(), self.yt.data_ptr(), self.partials.data_ptr(),
                self.partials.numel() * 4, self.B, cfg.n_head, cfg.n_local_heads, cfg.head_dim, self.max_seq, self.code, st)
        if self._active is None:
            rc, what = self.L.teal_batched_decode_attention(*head, *tail), "teal_batched_decode_attention"
        else:
            rc, what = self.L.teal_batched_decode_attention_slots(*head, self._active, *tail), "teal_batched_decode_attention_slots"
        if rc != 0:
            _lib.check(rc, what)

    def _sample_row(self, b: int, logits: torch.Tensor, temperature, top_k, feed, st):
        args = (logits.data_ptr(), self.cfg.vocab_size, self.code, int(top_k or 0), float(temperature), self.rng_state[b].data_ptr(),
                self.tok_buf[b:].data_ptr(), self.pos_buf[b:].data_ptr(), self.history[b].data_ptr(), self.history.shape[1],
                self.ws.data_ptr(), self.ws.numel() * 4)
        if self._active is None:
            rc, what = self.L.teal_sample_topk_ws(*args, st), "teal_sample_topk (batched)"
        else:
            rc, what = self.L.teal_sample_topk_slot(*args, self._active, b, st), "teal_sample_topk_slot"
        if rc != 0:
            _lib.check(rc, what)

    def _step(self, ths_override: Optional[float] = None):
        """one step for all B sequences from tok_buf / pos_buf -> self.logits [B, vocab] (no host synchronisation)"""
        m, cfg, L, st = self.model, self.cfg, self.L, runtime.stream_ptr()

        def gemm(i, j, gin, lin0, lin1, Z, out):
            self.splits[i][j] = ns = self._gemm(gin, self._segs[i][PROJ_LAUNCHES[j][0]], lin0, lin1, Z, out, self.counts[i, j], st,
                                                self._tau_row(i, j))
            return ns

        self._walk(self.B, self.tok_buf.data_ptr(), gemm, lambda at, A, ns: self._attention(at, A, ns, st), st)
        ns = self._gemm(self._norm_in(m.norm.weight), self._lm_segs, m.output, None, self.dim, self.lm_slabs, None, st)
        rc = L.teal_batched_round_rows(self.lm_slabs.data_ptr(), ns, cfg.vocab_size, self.B, self.logits.data_ptr(), self.code, st)
        if rc != 0:
            _lib.check(rc, "teal_batched_round_rows (lm_head)")
        return self.logits

    def _tau_row(self, i: int, j: int) -> Optional[int]:
        """the address of layer i, launch j's per-slot threshold table, or None: the launch takes its segments' thresholds"""
        return None

    @torch.no_grad()
    def __call__(self, tokens: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        """tokens [B], pos [B] (ints; positions may differ) -> logits [B, vocab] (a view of the engine's buffer).  Writes KV row
        pos[b] of sequence b in every layer."""
        B = self.B
        assert tokens.numel() == B and pos.numel() == B
        self.tok_buf[:B].copy_(tokens.view(-1).to(torch.int32))
        self.pos_buf[:B].copy_(pos.view(-1).to(torch.int32))
        return self._step()

    # ---- sampling and the device-resident loop ----------------------------------------------------
    def _sample(self, temperature: float, top_k: Optional[int]):
        # tok_buf still holds the tokens this step was fed: each sequence's latest, which the processors count first
        self._draw(self.logits, self.cfg.vocab_size, self.B, temperature, top_k, self.rng_state, self.tok_buf, self.pos_buf, self.history,
                   True, st=runtime.stream_ptr())

    @torch.no_grad()
    def sample_first(self, logits_rows: torch.Tensor) -> torch.Tensor:
        """per-request sampling on: the B tokens after the prompts, one sampling launch over the prompt pass's last-position logits
        [B, vocab] under each sequence's own row of settings -> int32 [B].  Sequence b draws from a stream of its own, seed + B + b
        (decode_n's streams are seed + b from draw 0); position, history and the decode streams do not move."""
        rows = logits_rows.to(self.dtype).contiguous()
        assert rows.shape == (self.B, self.cfg.vocab_size)
        state = torch.tensor([[self._seed + self.B + b, 0] for b in range(self.B)], dtype=torch.int64).to(rows.device)
        tok = torch.zeros(self.B, dtype=torch.int32, device=rows.device)
        self._sampling().launch(rows, rows.shape[1], self.B, state, tok, None, None, 0)
        return tok

    def read_logprobs(self, n: int):
        """(lp [B, n], top_ids [B, n, top_n], top_lp [B, n, top_n]) of the tokens history[:, :n] — decode_n's"""
        return self._logprobs().read(slice(None), 0, n)

    def _loop_state(self):
        """what the captured step carries from replay to replay (the capture's warm-up step is undone on these)"""
        return [self.tok_buf, self.pos_buf, self.rng_state, self.history] + self._feature_loop_state()

    def _self_step(self, temperature, top_k):
        self._step()
        self._sample(temperature, top_k)

    def capture(self, temperature: float = 0.8, top_k: Optional[int] = 200):
        """hipGraph of one step for all B sequences: the forward pass and B sampler launches (each sequence's token, position and
        draw counter stay on the device).  The warm-up step's state is put back."""
        key = self._step_key(temperature, top_k) + self._feature_key()
        if self._graph is not None and self._graph_key == key:
            return self._graph
        g, _ = runtime.capture_graph(lambda: self._self_step(temperature, top_k), self._loop_state())
        self._graph, self._graph_key = g, key
        return g

    def manual_seed(self, seed: int):
        self._seed = int(seed)

    @torch.no_grad()
    def decode_n(self, first_tokens: torch.Tensor, pos, n: int, temperature: float = 0.8, top_k: Optional[int] = 200,
                 use_graph: bool = True, prompt_tokens=None) -> torch.Tensor:
        """n steps from first_tokens [B] at positions pos (int or [B]); returns the sampled tokens [B, n] (one read-back at the
        end).  Sequence b draws from its own stream (seed + b).  prompt_tokens (B sequences of ids; with logit processors on):
        each sequence's processor state starts over with these as its prompt — first_tokens are then counted as generated by
        the first step, like every token a step is fed."""
        B = self.B
        if prompt_tokens is not None and self._proc is not None:
            assert len(prompt_tokens) == B
            for b in range(B):
                self._proc.reset(b, prompt_tokens[b])
        pos_t = torch.as_tensor(pos).to(torch.int32).reshape(-1).cpu()
        pos_t = pos_t.expand(B) if pos_t.numel() == 1 else pos_t
        assert int(pos_t.max()) + n <= self.max_seq and n <= self.history.shape[1]
        self.tok_buf[:B].copy_(first_tokens.view(-1).to(torch.int32))
        self.pos_buf[:B].copy_(pos_t.to(self.pos_buf.device))
        self.rng_state.copy_(torch.tensor([[self._seed + b, 0] for b in range(B)], dtype=torch.int64))
        if use_graph:
            g = self.capture(temperature, top_k)
            for _ in range(n):
                g.replay()
        else:
            for _ in range(n):
                self._self_step(temperature, top_k)
        return self.history[:, :n].clone()

    # ---- reporting --------------------------------------------------------------------------------
    def kept_fractions(self) -> Dict[str, Dict[str, float]]:
        """of the last step: per projection, the mean over layers and sequences of the fraction of rows a sequence keeps
        ("per_seq") and the mean over layers of the fraction the union keeps ("union") — the rows the step read"""
        c = self.counts.view(len(self.model.layers), len(PROJ_LAUNCHES), 16, 3, 9).cpu()
        out = {}
        for j, (_, projs) in enumerate(PROJ_LAUNCHES):
            Z = self.inter if projs == ("down",) else self.dim
            for s, proj in enumerate(projs):
                per, uni = [], []
                for i in range(len(self.model.layers)):
                    tot = c[i, j, :self.splits[i][j], s].sum(0)
                    per.append(tot[:self.B].double().mean().item() / Z)
                    uni.append(tot[8].item() / Z)
                out[proj] = {"per_seq": sum(per) / len(per), "union": sum(uni) / len(uni)}
        return out

    def weight_bytes_per_step(self) -> int:
        """bytes of weights the last step streamed: every projection's union rows x its row width, plus the dense lm_head"""
        c = self.counts.view(len(self.model.layers), len(PROJ_LAUNCHES), 16, 3, 9).cpu()
        es = self.model.output.weight.element_size()
        widths = {"q": self.dim, "k": self.kv, "v": self.kv, "o": self.dim, "gate": self.inter, "up": self.inter, "down": self.dim}
        total = 0
        for i in range(len(self.model.layers)):
            for j, (_, projs) in enumerate(PROJ_LAUNCHES):
                for s, proj in enumerate(projs):
                    total += int(c[i, j, :self.splits[i][j], s, 8].sum()) * widths[proj] * es
        return total + self.dim * self.cfg.vocab_size * es

    @property
    def config(self):
        return self.cfg

    @property
    def device(self):
        return self.logits.device


# ---- continuous batching: slots that drop out of the step on the device ---------------------------------------------------
# The slot state (include/teal_hip.h, TEAL_SLOT_*): one int32 buffer per engine, word offsets below.
SLOT_ACTIVE, SLOT_STEP, SLOT_BUDGET, SLOT_PRODUCED, SLOT_EOS, SLOT_FINISH, SLOT_WORDS = 0, 1, 8, 16, 24, 32, 40


class _SlotCacheView(torch.nn.Module):
    """slot s of a [B, n_kv, max_seq, hd] KVCache as a batch-1 cache: KVCache.update writes through the view into slot s only (a
    batch-1 update of the batch-B cache itself would broadcast the rows into every slot)."""

    def __init__(self, kv_cache, s: int):
        super().__init__()
        self.k_cache, self.v_cache = kv_cache.k_cache[s:s + 1], kv_cache.v_cache[s:s + 1]

    def update(self, input_pos, k_val, v_val):
        assert input_pos.shape[0] == k_val.shape[2]
        self.k_cache[:, :, input_pos] = k_val
        self.v_cache[:, :, input_pos] = v_val
        return self.k_cache, self.v_cache


class SlotPrefillEngine(_SlotCaches, PrefillEngine):
    """The HIP prompt pass (2..16 tokens) of one request into slot `slot` of batch-B caches: slot s of a contiguous
    [B, n_kv, max_seq, hd] cache is itself a contiguous [1, n_kv, max_seq, hd] cache, so the pass gets its base pointers."""

    @staticmethod
    def supports(model: Transformer) -> Optional[str]:
        return PrefillEngine._supports(model, any_batch=True)


class SlotVerifyPass(_SlotCaches, VerifyPass):
    """The dense pass over T <= 16 tokens at positions p .. p+T-1 (VerifyPass: p on the device, attention against the rows already
    in the cache) into slot `slot` of batch-B caches — the suffix pass of a request admitted on a shared prefix."""

    @staticmethod
    def supports(model: Transformer) -> Optional[str]:
        why = PrefillEngine._supports(model, any_batch=True)
        if why is None and model.config.vocab_size % 256:
            why = f"vocab_size {model.config.vocab_size} is not a multiple of 256 (the all-row lm_head GEMM's column contract)"
        return why

    def __init__(self, model: Transformer):
        super().__init__(model)
        self.rows = torch.zeros(8, 2 * model.config.vocab_size, device=self.lm_slabs.device, dtype=model.output.weight.dtype)

    def last_logits(self, ns: int, T: int) -> torch.Tensor:
        """logits [vocab] of row T - 1 from the `ns` lm_head slabs run() left: summed in slice order, rounded once"""
        V, st = self.model.config.vocab_size, runtime.stream_ptr()
        # slabs [ns][V][8] (T <= 8), or [ns][V][16] read as [ns][2 V][8]: column 2 v + j holds rows 8 j .. 8 j + 7 of logit v
        N, B = (V, T) if T <= 8 else (2 * V, 8)
        rc = self.L.teal_batched_round_rows(self.lm_slabs.data_ptr(), ns, N, B, self.rows.data_ptr(), self.code, st)
        if rc != 0:
            _lib.check(rc, "teal_batched_round_rows (suffix lm_head)")
        flat = self.rows.view(-1)
        if T <= 8:
            return flat[(T - 1) * V:T * V]
        return flat[((T - 1) % 8) * N:((T - 1) % 8 + 1) * N].view(V, 2)[:, (T - 1) // 8].contiguous()


class _Prefix:
    """one registered prefix: its K / V rows [2 L][n_kv][P][hd] (K, V of layer 0, K, V of layer 1, ...), the device table of the 2 L
    tensors' addresses and the position of a suffix's first token as a device int32"""

    def __init__(self, rows: int, store: torch.Tensor, tokens=()):
        self.rows, self.store, self.tokens = rows, store, [int(t) for t in tokens]  # (tokens: a request's prompt bits cover them)
        self.table = torch.tensor([store[t].data_ptr() for t in range(store.shape[0])], dtype=torch.int64).to(store.device)
        self.pos = torch.tensor([rows], dtype=torch.int32).to(store.device)


class SlotDecodeEngine(BatchedDecodeEngine):
    """BatchedDecodeEngine whose B slots are switched on and off on the device (continuous batching).  One hipGraph replay is the
    forward pass through the `_slots` launches (an inactive slot adds nothing to the union and writes no cache row), B
    slot-predicated samplers and teal_batched_retire, which counts each active slot's token and switches the slot off on its EOS
    id, its budget or the cache end.  `admit` puts one request into a free slot between replays.  With stop conditions on
    (set_stop_conditions) teal_batched_retire_stops takes the retire launch's place: stop ids, stop sequences, a minimum length
    and a finish reason per request (stopping.py).  With constraints on (set_constraints) one more launch in front of the samplers
    steps each slot's token automaton and masks the row it draws from (constraints.py).  With forced tokens on (set_forced_tokens)
    one more launch behind the samplers puts a request's given tokens in the drawn ones' place (forcing.py)."""

    _stops: Optional[ST.StopConditions] = None   # set_stop_conditions
    tau_table: Optional[torch.Tensor] = None     # set_slot_sparsity: fp32 [n_layer][4 launches][3][8] (None while it is off)
    _kv_kind = "slot"
    kv8 = None                                   # kv_cache="fp8": per layer (k codes, v codes, k scales, v scales)

    @staticmethod
    def supports(model: Transformer, kv_cache: Optional[str] = None) -> Optional[str]:
        """None if the slot step can run `model` as it stands, else the reason.  kv_cache None: batch = the caches' max_batch_size.
        "fp8": the model's caches are the staging cache, setup_caches(max_batch_size=1); the batch is the constructor's."""
        why = kv_cache_refusal("slot", kv_cache) or BatchedDecodeEngine.supports(model)
        cache_b = model.layers[0].attention.kv_cache.k_cache.shape[0] if why is None else 1
        if kv_cache is not None and cache_b != 1:
            why = (f"kv_cache={kv_cache!r} keeps the model's own caches as the staging cache of the prompt passes, the only 16-bit K / V "
                   f"left: setup_caches(max_batch_size=1), not {cache_b} (the engine owns the slots' fp8 rows)")
        return why

    def __init__(self, model: Transformer, thresholds: List[Dict[str, float]], batch: int, kv_cache: Optional[str] = None):
        """kv_cache None: the B slots are the model's own [B, n_kv, max_seq, hd] caches — every launch and allocation as without the
        keyword.  "fp8": the engine owns the slots' K / V as e4m3fn codes [B, n_kv, max_seq, hd] and power-of-two scales
        [B, n_kv, max_seq] per layer (include/teal_hip.h, "fp8 KV cache"); the model's caches, batch 1, are the staging cache every
        prompt pass writes, and one teal_kv8_quantize_rows launch per admission moves the prompt's rows into the slot.  A row is
        attended exactly by the pass that makes it (the prompt pass, a step's own new row) and as fp8 by every later step."""
        if kv_cache is not None:  # (the format, then the staging cache: checked here, before the batched engine's own checks)
            why = SlotDecodeEngine.supports(model, kv_cache=kv_cache)
            if why is not None:
                raise ValueError(f"SlotDecodeEngine cannot run this model: {why}")
        super().__init__(model, thresholds, batch, kv_cache)
        dev = self.logits.device
        self.slot_state = torch.zeros(SLOT_WORDS, dtype=torch.int32, device=dev)
        self.slot_state[SLOT_EOS:SLOT_EOS + 8] = -1
        self.slot_state[SLOT_FINISH:SLOT_FINISH + 8] = -1
        self._state_host = torch.zeros(SLOT_WORDS, dtype=torch.int32).pin_memory()
        self._prefill: Optional[SlotPrefillEngine] = None
        self._union = []  # per burst: union rows [layer][launch][segment] of the burst's last step
        self.admit_paths = {"hip": 0, "module": 0}
        # shared prefixes: per slot the device table of its 2 L cache tensors' addresses (K, V of layer 0, K, V of layer 1, ...)
        caches = [c for layer in model.layers for c in (layer.attention.kv_cache.k_cache, layer.attention.kv_cache.v_cache)]
        table = lambda ts, s: torch.tensor([t[s].data_ptr() for t in ts], dtype=torch.int64).to(dev)  # noqa: E731
        # (fp8: the one 16-bit "slot" is the staging cache; the slots proper are the code and scale tensors below)
        self._slot_tables = [table(caches, s) for s in range(caches[0].shape[0])]
        if kv_cache is not None:
            cfg = self.cfg
            shape = (self.B, cfg.n_local_heads, self.max_seq)
            # per layer (k codes, v codes, k scales, v scales); a scale of 1 under rows nobody wrote yet
            self.kv8 = [(torch.zeros(*shape, self.hd, dtype=torch.uint8, device=dev), torch.zeros(*shape, self.hd, dtype=torch.uint8, device=dev),
                         torch.ones(*shape, dtype=torch.float32, device=dev), torch.ones(*shape, dtype=torch.float32, device=dev))
                        for _ in model.layers]
            self._kv8_of = {id(layer.attention): i for i, layer in enumerate(model.layers)}
            codes = [c for kc, vc, _, _ in self.kv8 for c in (kc, vc)]
            scales = [c for _, _, ks, vs in self.kv8 for c in (ks, vs)]
            self._code_tables = [table(codes, s) for s in range(self.B)]
            self._scale_tables = [table(scales, s) for s in range(self.B)]
        self._prefixes: Dict[str, _Prefix] = {}
        self._verify: Optional[SlotVerifyPass] = None
        self._verify_why: Optional[str] = None
        self.prefix_paths = {"hip": 0, "module": 0}
        self.admit_logits: Optional[torch.Tensor] = None

    @property
    def _active(self) -> int:
        return self.slot_state.data_ptr()

    def _attention(self, at, A: torch.Tensor, ns: int, st):
        if self.kv8 is None:
            return super()._attention(at, A, ns, st)
        cfg = self.cfg
        kc, vc, ks, vs = self.kv8[self._kv8_of[id(at)]]
        rc = self.L.teal_batched_decode_attention_slots_kv8(
            A.data_ptr(), ns, self.rope.data_ptr(), self.pos_buf.data_ptr(), self._active, kc.data_ptr(), vc.data_ptr(), ks.data_ptr(),
            vs.data_ptr(), self.yt.data_ptr(), self.partials.data_ptr(), self.partials.numel() * 4, self.B, cfg.n_head, cfg.n_local_heads,
            cfg.head_dim, self.max_seq, self.code, st)
        if rc != 0:
            _lib.check(rc, "teal_batched_decode_attention_slots_kv8")

    def _quantize_rows(self, s: int, rows: int):
        """rows 0 .. rows-1 of the staging cache (every layer's K and V) into slot s's codes and scales: one launch"""
        rc = self.L.teal_kv8_quantize_rows(self._slot_tables[0].data_ptr(), self._code_tables[s].data_ptr(), self._scale_tables[s].data_ptr(),
                                           2 * len(self.model.layers), self.cfg.n_local_heads, self.hd, rows, self.max_seq, self.max_seq,
                                           self.code, runtime.stream_ptr())
        if rc != 0:
            _lib.check(rc, "teal_kv8_quantize_rows")

    def _cache_slot(self, s: int) -> int:
        """the slot of the model's caches a prompt pass for slot s writes: s itself, or the staging cache's only one"""
        return s if self.kv8 is None else 0

    def kv_cache_bytes(self) -> Dict[str, int]:
        """bytes of K / V the engine's slots hold, by kind.  staging: the model's own 16-bit caches (kv_cache None: they ARE the B
        slots; "fp8": the one sequence the prompt passes write).  codes / scales: the slots' fp8 rows (0 without them)."""
        nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)  # noqa: E731
        staging = nbytes(c for layer in self.model.layers for c in (layer.attention.kv_cache.k_cache, layer.attention.kv_cache.v_cache))
        kv8 = self.kv8 or []
        return {"staging": staging, "codes": nbytes(c for t in kv8 for c in t[:2]), "scales": nbytes(c for t in kv8 for c in t[2:])}

    def _retire(self, mask: int, count_step: bool, st):
        if self._stops is not None:  # the same place in the step, one launch for one
            self._stops.launch(self._active, self.tok_buf, self.pos_buf, self.history, self.B, mask, self.max_seq, count_step, st=st)
            return
        rc = self.L.teal_batched_retire(self._active, self.tok_buf.data_ptr(), self.pos_buf.data_ptr(), self.B, mask, self.max_seq,
                                        int(count_step), st)
        if rc != 0:
            _lib.check(rc, "teal_batched_retire")

    def _sample(self, temperature: float, top_k: Optional[int]):
        super()._sample(temperature, top_k)  # (an inactive slot counts nothing, draws nothing and records nothing)
        self._retire((1 << self.B) - 1, True, runtime.stream_ptr())

    def _loop_state(self):
        # the warm-up step retires too (and, with stop conditions on, writes a stopped slot's REASON and MATCH)
        return super()._loop_state() + [self.slot_state] + (list(self._stops.loop_tensors()) if self._stops is not None else [])

    def _feature_key(self):
        return super()._feature_key() + (("stops",) if self._stops is not None else ()) + \
               (("slot sparsity",) if self.tau_table is not None else ()) + ((f"kv {self.kv_cache}",) if self.kv_cache is not None else ())

    # ---- stop conditions ---------------------------------------------------------------------------------------------------
    def set_stop_conditions(self, on: bool):
        """off (the default): every step and every admission issues exactly the launches it issues without this feature.  on:
        teal_batched_retire_stops takes teal_batched_retire's place in the step and in admit's first draw — a slot also ends on
        its request's stop ids and stop sequences, none of them (nor its EOS id) before its min_new_tokens, and read_finish tells
        why it ended.  Allowed on an idle engine only (a running slot's row would be empty); drops the captured graphs."""
        if int(self.slot_state[SLOT_ACTIVE].item()) != 0:
            raise RuntimeError("set_stop_conditions needs an idle engine: a slot is active")
        self._stops = ST.StopConditions(self.B, self.cfg.vocab_size, self.history.device) if on else None
        self._graph = None

    def _stop_conditions(self) -> ST.StopConditions:
        if self._stops is None:
            raise RuntimeError("stop conditions are off (set_stop_conditions)")
        return self._stops

    # the stop table int32 [8][TEAL_STOP_WORDS] (None while the feature is off)
    stop_table = property(lambda self: None if self._stops is None else self._stops.table)

    def read_finish(self, slot: int):
        """(reason, match) of the request that last stopped in `slot`: "stop_token" (match: the token id), "stop_sequence" (match:
        the sequence's index), "length" or "cache" (match: -1); (None, -1) while it runs"""
        if not 0 <= int(slot) < self.B:
            raise ValueError(f"slot {slot} outside 0..{self.B - 1}")
        return self._stop_conditions().read()[int(slot)]

    # ---- per-request sparsity ----------------------------------------------------------------------------------------------
    def set_slot_sparsity(self, on: bool):
        """off (the default): every step and every admission issues exactly the launches it issues without this feature.  on: the
        layers' GEMM launches are teal_batched_sparse_gemm_slot_taus — slot b keeps a row under its OWN threshold, column b of the
        launch's table [segment][slot] — and admit(..., thresholds=) writes a request's column; every column starts at the engine's
        own thresholds.  The lm_head launch keeps every row either way.  A step streams the union of the rows its active slots keep,
        each under its own thresholds.  Allowed on an idle engine only (a running slot's column would be reset); drops the captured
        graphs."""
        if int(self.slot_state[SLOT_ACTIVE].item()) != 0:
            raise RuntimeError("set_slot_sparsity needs an idle engine: a slot is active")
        self.tau_table = None
        if on:
            cols = torch.tensor([self._tau_column(self.ths)] * 8, dtype=torch.float32)   # [slot][layer][launch][segment]
            self.tau_table = cols.permute(1, 2, 3, 0).contiguous().to(self.logits.device)
            assert self.tau_table.data_ptr() % 32 == 0
        self._graph = None

    @staticmethod
    def _tau_column(ths) -> List[List[List[float]]]:
        """[layer][launch][segment] of one slot's column: the launch's thresholds in segment order, absent segments at +inf"""
        return [[[float(t[p]) for p in projs] + [math.inf] * (3 - len(projs)) for _, projs in PROJ_LAUNCHES] for t in ths]

    def _check_thresholds(self, thresholds) -> List[Dict[str, float]]:
        """a request's thresholds, refused (ValueError with the reason) unless one dict per layer holds a number that is not NaN
        under every key of the constructor's"""
        ths = list(thresholds)
        if len(ths) != len(self.ths):
            raise ValueError(f"thresholds: {len(ths)} dicts for {len(self.ths)} layers (one per layer)")
        for i, t in enumerate(ths):
            for p in PROJ_KEYS:
                if p not in t:
                    raise ValueError(f"thresholds: layer {i} has no {p!r} (keys {', '.join(PROJ_KEYS)})")
                if math.isnan(float(t[p])):
                    raise ValueError(f"thresholds: layer {i} {p!r} is NaN")
        return ths

    def _tau_row(self, i: int, j: int) -> Optional[int]:
        return None if self.tau_table is None else self.tau_table[i, j].data_ptr()

    def kept_by_slot(self) -> Dict[str, List[float]]:
        """of the last step: per projection, for each slot the fraction of rows it kept, the mean over layers (0 for a slot that
        did not run) — the counts kept_fractions() averages over the slots"""
        c = self.counts.view(len(self.model.layers), len(PROJ_LAUNCHES), 16, 3, 9).cpu()
        out = {}
        for j, (_, projs) in enumerate(PROJ_LAUNCHES):
            Z = self.inter if projs == ("down",) else self.dim
            for s, proj in enumerate(projs):
                tot = sum(c[i, j, :self.splits[i][j], s].sum(0)[:self.B].double() for i in range(len(self.model.layers)))
                out[proj] = (tot / (Z * len(self.model.layers))).tolist()
        return out

    # ---- constraints -------------------------------------------------------------------------------------------------------
    def set_constraints(self, on: bool, capacity_words: int = 1 << 20):
        """off (the default): every step and every admission issues exactly the launches it issues without this feature.  on: one
        launch between the logit processors (if on) and the samplers steps each slot's token automaton on the token the step was
        fed and bans, in the row the samplers read, every token the automaton's state does not allow (admit(..., constraint=);
        slots without one are copied bit for bit).  capacity_words: the arena the registered automata's images share.  Allowed on
        an idle engine only (a running slot's automaton would start in the middle of its output); drops the captured graphs and
        every registered constraint."""
        if int(self.slot_state[SLOT_ACTIVE].item()) != 0:
            raise RuntimeError("set_constraints needs an idle engine: a slot is active")
        self._con = CN.Constraints(self.B, self.cfg.vocab_size, self.dtype, self.history.shape[-1], self.history.device,
                                   capacity_words) if on else None
        self._graph = None

    def _eos_words(self, row0: int) -> int:
        return self.slot_state.data_ptr() + 4 * (SLOT_EOS + row0)

    # ---- forced tokens -----------------------------------------------------------------------------------------------------
    def set_forced_tokens(self, on: bool, capacity: Optional[int] = None):
        """off (the default): every step and every admission issues exactly the launches it issues without this feature.  on: one
        launch between the samplers and the logprob launch puts, for draws 0 .. n-1 of a request admitted with n forced tokens
        (admit(..., forced_tokens=)), the given token in the drawn one's place — in the token word and the history entry, the only
        two words that name it: the logprob, the retire rule, the next step and its logit processors see the forced token as the
        drawn one.  capacity: the forced tokens a request may carry (default: max_seq); the table is int32 [8][capacity] with a
        length word per slot, all 0, written by admissions only — nothing of it joins the loop state.  Allowed on an idle engine
        only (a running slot's row would be empty); drops the captured graphs."""
        if int(self.slot_state[SLOT_ACTIVE].item()) != 0:
            raise RuntimeError("set_forced_tokens needs an idle engine: a slot is active")
        self._frc = FT.ForcedTokens(self.B, self.max_seq if capacity is None else capacity, self.cfg.vocab_size,
                                    self.history.device) if on else None
        self._graph = None

    def read_forced(self, slot: int) -> int:
        """the length word of `slot`: how many tokens its last admission forced (0: none)"""
        if not 0 <= int(slot) < self.B:
            raise ValueError(f"slot {slot} outside 0..{self.B - 1}")
        return self._forced().read(int(slot))

    def register_constraint(self, name: str, automaton: CN.Automaton):
        """the automaton's image into the arena under `name`, for admit(..., constraint=name).  It is checked at this engine's
        vocabulary here (ValueError with the reason) and against each request's own EOS id at its admission.  Allowed while slots
        run: the arena's free blocks are no running slot's."""
        con = self._constraints()
        if not isinstance(automaton, CN.Automaton):
            raise ValueError(f"register_constraint takes an Automaton, got {type(automaton).__name__}")
        automaton.check(self.cfg.vocab_size, None, eos_known=False)
        con.register(name, automaton)

    def drop_constraint(self, name: str):
        """frees the image; refused (RuntimeError) while a running slot names it"""
        con = self._constraints()
        state = int(self.slot_state[SLOT_ACTIVE].item())
        for s, n in enumerate(con.row_names):  # a finished slot's row still names its last constraint: it lets go here
            if n == name and not (state >> s) & 1:
                con.set_row(s, None)
        torch.cuda.current_stream().synchronize()  # (a launch that reads the image may still be in flight)
        con.drop(name)

    def has_constraint(self, name: str) -> bool:
        return self._con is not None and name in self._con.images

    def read_constraint_trace(self, slot: int, n: int) -> List[int]:
        """the automaton states draws 0 .. n-1 of the request in `slot` were made in (bit 30 set: the fed token was banned —
        cannot happen for tokens drawn under the mask); all 0 for an unconstrained request"""
        if not 0 <= int(slot) < self.B:
            raise ValueError(f"slot {slot} outside 0..{self.B - 1}")
        return self._constraints().read_trace(slot, n)

    # ---- admission ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _prompt_pass(self, s: int, prompt: torch.Tensor) -> torch.Tensor:
        """the dense prompt pass of one request into slot s's caches only (fp8: into the staging cache) -> logits [vocab] of its last
        token"""
        T = int(prompt.numel())
        m = self.model
        if 2 <= T <= MAX_T:  # the HIP prompt pass at the slot's cache base pointers
            if self._prefill is None:
                self._prefill = SlotPrefillEngine(m)
            self._prefill.slot = self._cache_slot(s)
            self.admit_paths["hip"] += 1
            return self._prefill(prompt.to(torch.int32)).view(-1)
        # the module path on a batch-1 view of slot s (the op-by-op ops: a one-token prompt takes the sparse kernels, a longer
        # one the dense matmul, as generate()'s module path does)
        self.admit_paths["module"] += 1
        return self._module_pass(s, prompt, 0)

    def _module_pass(self, s: int, prompt: torch.Tensor, start: int) -> torch.Tensor:
        """the module path over `prompt` at positions start .. start+T-1 on a batch-1 view of slot s -> logits [vocab] of the last"""
        T = int(prompt.numel())
        m = self.model
        saved = [layer.attention.kv_cache for layer in m.layers]
        fused = m.fused_decode
        try:
            for layer, kc in zip(m.layers, saved):
                layer.attention.kv_cache = _SlotCacheView(kc, self._cache_slot(s))
            m.fused_decode = False
            logits = m(prompt.view(1, -1), torch.arange(start, start + T, device=prompt.device))
        finally:
            for layer, kc in zip(m.layers, saved):
                layer.attention.kv_cache = kc
            m.fused_decode = fused
        return logits[0, -1].contiguous()

    # ---- shared prefixes ---------------------------------------------------------------------------------------------------
    def _copy_rows(self, src_table: torch.Tensor, dst_table: torch.Tensor, rows: int, src_rows: int, dst_rows: int):
        """rows 0 .. rows-1 of every head of the 2 L tensors of one table into the other's (heads of src_rows / dst_rows rows)"""
        rb = self.hd * self.model.output.weight.element_size()
        rc = self.L.teal_kv_copy_rows(src_table.data_ptr(), dst_table.data_ptr(), 2 * len(self.model.layers), self.cfg.n_local_heads,
                                      rows, rb, src_rows * rb, dst_rows * rb, runtime.stream_ptr())
        if rc != 0:
            _lib.check(rc, "teal_kv_copy_rows")

    @torch.no_grad()
    def register_prefix(self, name: str, tokens) -> int:
        """Computes the K / V rows of `tokens` once — the prompt pass admitting them would run, into slot 0's caches — and keeps
        them in a device store [2 L][n_kv][P][hd] under `name`; returns P.  The engine must be idle (slot 0's cache rows 0 .. P-1
        are overwritten); no slot state, token, position, history or rng state moves and admit_paths does not count it."""
        if name in self._prefixes:
            raise ValueError(f"prefix {name!r} is registered already")
        if int(self.slot_state[SLOT_ACTIVE].item()) != 0:
            raise RuntimeError("register_prefix needs an idle engine: a slot is active")
        toks = torch.as_tensor(tokens, dtype=torch.int32).view(-1).to(self.logits.device)
        P = int(toks.numel())
        if P < 1 or P + 1 >= self.max_seq:
            raise ValueError(f"prefix {name!r} of {P} tokens leaves no room for a suffix in a cache of {self.max_seq} rows")
        counted = dict(self.admit_paths)
        try:
            self._prompt_pass(0, toks)
        finally:
            self.admit_paths = counted
        store = torch.empty(2 * len(self.model.layers), self.cfg.n_local_heads, P, self.hd, device=self.logits.device, dtype=self.dtype)
        pf = _Prefix(P, store, toks.tolist())
        self._copy_rows(self._slot_tables[0], pf.table, P, self.max_seq, P)
        self._prefixes[name] = pf
        return P

    def drop_prefix(self, name: str):
        if name not in self._prefixes:
            raise ValueError(f"unknown prefix {name!r}")
        torch.cuda.current_stream().synchronize()  # (a copy out of the store may still be in flight)
        del self._prefixes[name]

    def has_prefix(self, name: str) -> bool:
        return name in self._prefixes

    def prefix_rows(self, name: str) -> int:
        return self._prefixes[name].rows

    def prefix_store(self, name: str) -> torch.Tensor:
        """the store [2 L][n_kv][P][hd]: K, V of layer 0, K, V of layer 1, ..."""
        return self._prefixes[name].store

    def prefix_bytes(self) -> int:
        return sum(p.store.numel() * p.store.element_size() for p in self._prefixes.values())

    def _suffix_pass(self, s: int, pf: _Prefix, suffix: torch.Tensor) -> torch.Tensor:
        """the prefix's rows into slot s (one launch), then the dense pass over the suffix at positions P .. P+T-1 into slot s's
        caches only -> logits [vocab] of its last token"""
        T = int(suffix.numel())
        self._copy_rows(pf.table, self._slot_tables[self._cache_slot(s)], pf.rows, pf.rows, self.max_seq)
        if T <= MAX_T and self._verify is None and self._verify_why is None:
            self._verify_why = SlotVerifyPass.supports(self.model)
            if self._verify_why is None:
                self._verify = SlotVerifyPass(self.model)
        if T <= MAX_T and self._verify is not None:  # the HIP verify pass at the slot's cache base pointers
            self._verify.slot = self._cache_slot(s)
            self.prefix_paths["hip"] += 1
            return self._verify.last_logits(self._verify.run(suffix, pf.pos, T), T)
        self.prefix_paths["module"] += 1
        return self._module_pass(s, suffix, pf.rows)

    @torch.no_grad()
    def admit(self, slot: int, tokens, budget: int, eos_id: Optional[int], seed: int, temperature: float = 0.8,
              top_k: Optional[int] = 200, prefix: Optional[str] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
              frequency_penalty: float = 0.0, logit_bias: Optional[Dict] = None, top_p: float = 1.0, min_p: float = 0.0,
              stop_token_ids=(), stop_sequences=(), min_new_tokens: int = 0, constraint: Optional[str] = None,
              thresholds: Optional[List[Dict[str, float]]] = None, forced_tokens=()):
        """Request -> slot `slot` (free): the dense prompt pass into that slot's caches, the first token drawn from the last row's
        logits (draw 0 of the stream `seed`), the slot's token, position, history, rng state, budget and EOS set on the device and
        its bit set.  A request whose first token ends it (budget 1, EOS) is switched off again by the same retire rule.
        `prefix`: a registered prefix of P rows — `tokens` are the request's own suffix; the store's rows 0 .. P-1 are copied into
        the slot and only the suffix is run, at positions P .. P+T-1: the request is served as prompt = prefix + suffix.
        repetition_penalty / presence_penalty / frequency_penalty / logit_bias: the request's logit processors (they need
        set_logit_processors(True); its prompt tokens — prefix + suffix — are marked, and every token it draws, the first
        included, passes through them).
        top_p / min_p: nucleus and min-p sampling of this request (they need set_sampling_params(True)).  With per-request sampling
        on, `temperature`, `top_k`, `top_p` and `min_p` are written into the slot's parameter row and hold for every draw of the
        request; off, `temperature` and `top_k` are those of this first draw only (run_steps has its own).
        stop_token_ids / stop_sequences / min_new_tokens: the request's stop conditions (they need set_stop_conditions(True)): up
        to 16 ids, up to 8 sequences of up to 8 token ids, matched against the tokens it generates — never its prompt or prefix;
        neither they nor `eos_id` end it before min_new_tokens tokens.  The stopping tokens stay in its output.
        constraint: a registered constraint's name (it needs set_constraints(True)) — every token of the request, the first
        included, is drawn from the tokens its automaton allows, and `eos_id` only in an accepting state.  The automaton is checked
        against this request's `eos_id` here; a temperature above 100 is refused (a banned token's weight must be exactly 0).
        thresholds: the request's own sparsity level, one dict per layer with the constructor's keys (it needs
        set_slot_sparsity(True)); None: the engine's own.  With the feature on every admission writes the slot's whole column.
        forced_tokens: token ids the request's draws 0 .. n-1 yield in place of what its sampler drew (they need
        set_forced_tokens(True)): at most the table's capacity and at most `budget`, never together with `constraint` (a forced
        token may be one the automaton bans).  A forced token is a drawn token for every rule that follows — EOS, stop conditions,
        budget, processors — and its logprob is the model's for that token.  A larger budget goes on sampling after the last one,
        from the stream where the draw counter stands.  With the feature on every admission writes the slot's length word."""
        s, B = int(slot), self.B
        prompt = torch.as_tensor(tokens, dtype=torch.int32).view(-1).to(self.logits.device)
        T = int(prompt.numel())
        if not 0 <= s < B:
            raise ValueError(f"slot {s} outside 0..{B - 1}")
        pf = None
        if prefix is not None:
            pf = self._prefixes.get(prefix)
            if pf is None:
                raise ValueError(f"unknown prefix {prefix!r} (register_prefix first)")
        P = pf.rows if pf is not None else 0
        if T < 1 or P + T >= self.max_seq or int(budget) < 1:
            raise ValueError(f"request of {T} prompt tokens" + (f" on a prefix of {P}" if pf is not None else "") +
                             f" and budget {budget} does not fit a cache of {self.max_seq} rows")
        controls = PR.check_controls(self.cfg.vocab_size, repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
        if self._proc is None and not PR.is_identity(controls):
            raise RuntimeError("logit processors are off (set_logit_processors)")
        stops = ST.check_stops(self.cfg.vocab_size, stop_token_ids, stop_sequences, min_new_tokens)
        if self._stops is None and not ST.is_default(stops):
            raise RuntimeError("stop conditions are off (set_stop_conditions)")
        if constraint is not None:
            if self._con is None:
                raise RuntimeError("constraints are off (set_constraints)")
            self._con.automaton(constraint).check(self.cfg.vocab_size, eos_id)
            if float(temperature) > CN.MAX_TEMPERATURE:
                raise ValueError(f"a constrained request needs temperature <= {CN.MAX_TEMPERATURE:g} (above it a banned token's weight "
                                 f"is no longer exactly 0), got {temperature}")
        if thresholds is not None:
            if self.tau_table is None:
                raise RuntimeError("per-request sparsity is off (set_slot_sparsity)")
            thresholds = self._check_thresholds(thresholds)
        forced = FT.check_forced(self.cfg.vocab_size, forced_tokens)
        if forced:
            if self._frc is None:
                raise RuntimeError("forced tokens are off (set_forced_tokens)")
            if len(forced) > self._frc.capacity:
                raise ValueError(f"{len(forced)} forced tokens: the table holds {self._frc.capacity} per request (set_forced_tokens(capacity=))")
            if len(forced) > int(budget):
                raise ValueError(f"{len(forced)} forced tokens exceed the request's budget of {int(budget)}")
            if constraint is not None:
                raise ValueError("forced tokens do not combine with a constraint: a forced token may be one the automaton bans")
        if self._samp is not None:
            SM.check_sampling(temperature, top_k, top_p, min_p)
        elif SM.check_sampling(top_p=top_p, min_p=min_p)["top_p"] < 1.0 or min_p > 0.0:
            raise RuntimeError("per-request sampling is off (set_sampling_params)")
        # Every refusal is above, every write to a device table below: a refused admission leaves the slot as it found it.  (But
        # for LogitProcessors.set_row's own: a bias that is not finite in the model dtype — it needs the device dtype — and a prompt
        # token outside the vocabulary are refused there, after the rows before it are written.)
        if self.tau_table is not None:  # (every admission: the slot's next occupant never inherits a level)
            col = torch.tensor(self._tau_column(self.ths if thresholds is None else thresholds), dtype=torch.float32)
            self.tau_table[..., s].copy_(col.to(self.tau_table.device))
        if self._frc is not None:  # (every admission: the slot's next occupant never inherits a row)
            self._frc.set_row(s, forced)
        if self._con is not None:  # (every admission: the slot's next occupant never inherits a constraint)
            self._con.set_row(s, constraint)
        if self._samp is not None:  # (every admission: the slot's last request left its settings)
            self._samp.set_row(s, temperature, top_k, top_p, min_p)
        if self._stops is not None:  # (every admission: the slot's last request left its row, and its reason)
            self._stops.set_row(s, **stops)
        if self._proc is not None:  # (every admission: the slot's last request left its counts and its parameters)
            self._proc.set_row(s, (pf.tokens if pf is not None else []) + prompt.tolist(), **controls)
        logits = self._prompt_pass(s, prompt) if pf is None else self._suffix_pass(s, pf, prompt)
        if self.kv8 is not None:  # the staging cache's rows 0 .. P+T-1 into the slot (outside the captured step)
            self._quantize_rows(s, P + T)
        self.admit_logits = logits  # (the last admission's, for tests and reports: valid until the next one)
        self.rng_state[s].copy_(torch.tensor([int(seed), 0], dtype=torch.int64), non_blocking=False)
        self.pos_buf[s] = P + T - 1  # the sampler moves it to P + T: the row the first decode step writes
        upd = torch.tensor([int(budget), 0, -1 if eos_id is None else int(eos_id), -1], dtype=torch.int32).to(self.slot_state.device)
        for j, off in enumerate((SLOT_BUDGET, SLOT_PRODUCED, SLOT_EOS, SLOT_FINISH)):
            self.slot_state[off + s:off + s + 1].copy_(upd[j:j + 1])
        self.slot_state[SLOT_ACTIVE:SLOT_ACTIVE + 1].bitwise_or_(1 << s)
        st = runtime.stream_ptr()
        # the first draw, entry 0 of the request's rows: nothing generated yet, so the processors count nothing
        self._draw(logits, 0, 1, temperature, top_k, self.rng_state[s], self.tok_buf[s:], self.pos_buf[s:], self.history[s], False,
                   row0=s, st=st)
        self._retire(1 << s, False, st)

    # ---- the batcher's view ------------------------------------------------------------------------------------------------
    def run_steps(self, k: int, temperature: float = 0.8, top_k: Optional[int] = 200, use_graph: bool = True):
        """k steps of every active slot (no host synchronisation); the union counts of the last are kept for the report"""
        if use_graph:
            g = self.capture(temperature, top_k)
            for _ in range(k):
                g.replay()
        else:
            for _ in range(k):
                self._self_step(temperature, top_k)
        self._union.append(self.counts.view(len(self.model.layers), len(PROJ_LAUNCHES), 16, 3, 9)[..., 8].sum(2))

    def read_state(self):
        """the slot state in one device-to-host copy (a list of SLOT_WORDS ints)"""
        self._state_host.copy_(self.slot_state, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self._state_host.tolist()

    def read_history(self, slot: int, n: int) -> List[int]:
        return self.history[slot, :n].tolist()

    def read_logprobs(self, slot: int, n: int):
        """(lp, top_ids, top_lp) of the tokens read_history(slot, n) returns, as lists: n floats, n lists of top_n ids, n lists of
        top_n floats"""
        lp, ids, tlp = self._logprobs().read(slot, 0, n)
        return lp.tolist(), ids.tolist(), tlp.tolist()

    def union_kept(self) -> Dict[str, float]:
        """per projection: the mean over layers and over the bursts whose last step had an active slot of the fraction of rows
        the union of the ACTIVE slots kept"""
        if not self._union:
            return {}
        u = torch.stack(self._union).cpu().double()  # [bursts, layer, launch, segment]
        live = u.flatten(1).sum(1) > 0
        u = u[live]
        out = {}
        if u.shape[0] == 0:
            return out
        for j, (_, projs) in enumerate(PROJ_LAUNCHES):
            Z = self.inter if projs == ("down",) else self.dim
            for s, proj in enumerate(projs):
                out[proj] = u[:, :, j, s].mean().item() / Z
        return out

    def reset_stats(self):
        self._union = []
        self.admit_paths = {"hip": 0, "module": 0}
        self.prefix_paths = {"hip": 0, "module": 0}
