#!/usr/bin/env python3
"""Decode harness with the reference's CLI surface (gpt-fast/generate.py:528-558):

    python -m teal_amd.gpt_fast.generate --checkpoint_path .../model.pth --hist_path models/Llama-2-7B/histograms \
        --sparsity 0.5 --compile
    python -m teal_amd.gpt_fast.generate --synthetic 7B --sparsity 0.5 --compile          (no checkpoint needed)

Same flags (`--hist_path`, `--sparsity`, `--checkpoint_path`, `--compile`, `--num_samples`,
`--max_new_tokens`, `--top_k`, `--temperature`, `--prompt`, `--profile`), same tokens/sec definition
(generated tokens / wall time of one generate() call INCLUDING prefill, one warm-up sample then
`num_samples` timed ones, generate.py:431-506), same seed (1234).  Differences, all MI355X-first:

  * `--compile` means "capture the decode step into a hipGraph" (torch.cuda.CUDAGraph), not
    torch.compile/Inductor/Triton: the sparse GEMVs are hand-written HIP behind torch.ops.teal.*,
    launch geometry is fixed by shape, so there is nothing to trace or autotune.
  * `--precision {fp16,bf16}` (reference hard-codes fp16, generate.py:386), `--greedy_lookup DIR`
    (wires utils.get_layer_greedy_sparsities, which the reference imports but never calls),
    `--synthetic NAME` (random weights of the named architecture + thresholds calibrated on the
    synthetic activations, because there is no network for checkpoints here), `--engine`
    (fused HIP decode step, teal_amd/gpt_fast/engine.py) and `--dense` (no monkeypatch: baseline).
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import itertools
import json
import os
import sys
import time
from pathlib import Path
from typing import Dict, List, Optional

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from teal_amd import runtime  # noqa: E402
from teal_amd.gpt_fast.engine_features import pointer_key, relayout  # noqa: E402
from teal_amd.gpt_fast.model import ModelArgs, Transformer  # noqa: E402
from teal_amd.monkeypatch import monkeypatch_layer  # noqa: E402
from teal_amd.utils import PROJS, get_layer_greedy_sparsities  # noqa: E402

default_device = "cuda" if torch.cuda.is_available() else "cpu"


# ------------------------------------------------------------------------------------------------
# sampling (gpt-fast/generate.py:49-66: top-k, softmax, exponential-trick multinomial, no host sync)
# ------------------------------------------------------------------------------------------------
def multinomial_sample_one_no_sync(probs_sort: torch.Tensor) -> torch.Tensor:
    q = torch.empty_like(probs_sort).exponential_(1)
    return torch.argmax(probs_sort / q, dim=-1, keepdim=True).to(dtype=torch.int)


def logits_to_probs(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None) -> torch.Tensor:
    logits = logits / max(temperature, 1e-5)
    if top_k is not None:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits = torch.where(logits < v.select(-1, -1).unsqueeze(-1), -float("Inf"), logits)
    return torch.nn.functional.softmax(logits, dim=-1)


def sample(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None):
    probs = logits_to_probs(logits[0, -1].float(), temperature, top_k)
    return multinomial_sample_one_no_sync(probs), probs


# ------------------------------------------------------------------------------------------------
# model construction
# ------------------------------------------------------------------------------------------------
def build_synthetic_model(name: str, device: str, dtype: torch.dtype, seed: int = 1234, std: float = 0.02,
                          n_layer: Optional[int] = None, shard=None) -> Transformer:
    """Random-init weights N(0, std^2) at the exact shapes of the named architecture.

    `shard(model)` (tensor parallelism: tp.apply_tp) runs on the META model, before any storage exists: a rank then
    allocates only its slices, and fills each from the full random tensor of that parameter — drawn in the unsharded order
    from the same seed, so the ranks' weights ARE the slices of the unsharded synthetic model (one fp32 temporary of the
    largest parameter at a time)."""
    cfg = ModelArgs.from_name(name)
    if n_layer is not None:
        cfg.n_layer = n_layer
    with torch.device("meta"):
        model = Transformer(cfg).to(dtype)
    full_shape = {pname: tuple(p.shape) for pname, p in model.named_parameters()}
    if shard is not None:
        shard(model)
    g = torch.Generator(device=device).manual_seed(seed)
    # storage is allocated ONCE, in the target dtype, and filled in place: Llama-2-70B peaks at its 137 GB of weights plus
    # one fp32 temporary (it used to materialise the fp32 meta model first: 279 GB reserved of the GPU's 288 GB)
    model = model.to_empty(device=device)
    owner = {id(m.weight): m for m in model.modules() if hasattr(m, "_tp")}
    with torch.no_grad():
        for pname, p in model.named_parameters():
            if pname.endswith("norm.weight"):
                p.data.fill_(1.0)
                continue
            w = torch.randn(full_shape[pname], device=device, dtype=torch.float32, generator=g) * std
            if id(p) in owner:  # this rank's rows (column-wise) or columns (row-wise) of the full tensor
                style, ranges = owner[id(p)]._tp
                w = torch.cat([w.narrow(0 if style == "colwise" else 1, lo, hi - lo) for lo, hi in ranges], dim=0 if style == "colwise" else 1)
            p.data.copy_(w)
            del w
    return model.eval()


def load_checkpoint_model(checkpoint_path: Path, device: str, dtype: torch.dtype, shard=None) -> Transformer:
    """`shard(model)` (tensor parallelism: tp.apply_tp) runs on the memory-mapped CPU tensors right after the state dict is
    assigned — before anything moves to the device — like the reference (gpt-fast/generate.py:249-256)."""
    with torch.device("meta"):
        model = Transformer.from_name(checkpoint_path.parent.name)
    if "int8" in str(checkpoint_path):  # gpt-fast/generate.py:239-243: an int8 weight-only checkpoint (quantize.py --mode int8)
        from teal_amd.quantize import convert_for_runtime_int8
        print("Using int8 weight-only quantization!")
        convert_for_runtime_int8(model, dtype)
    int4 = "int4" in str(checkpoint_path)
    if int4:  # gpt-fast/generate.py:236-242: model_int4.g32.pth -> groupsize 32 (a checkpoint written by teal_amd.quantize:
        # quantize_model_int4(model).state_dict(); the reference's own int4 files hold a CUDA-only packed layout)
        from teal_amd.quantize import convert_for_runtime_int4
        groupsize = int(checkpoint_path.name.split(".")[-2][1:])
        print("Using int4 weight-only quantization!")
        convert_for_runtime_int4(model, groupsize)
    ckpt = torch.load(str(checkpoint_path), mmap=True, weights_only=True)
    if "model" in ckpt and "stories" in str(checkpoint_path):
        ckpt = ckpt["model"]
    model.load_state_dict(ckpt, assign=True)
    if shard is not None:
        shard(model)
    if int4:  # packed uint8 weights and bf16 group parameters stay as they are; everything else takes the activation dtype
        model = model.to(device=device)
        for prm in model.parameters():
            prm.data = prm.data.to(dtype)
        return model.eval()
    if "int8" in str(checkpoint_path):  # keep the int8 buffers int8: only floating tensors take the activation dtype
        model = model.to(device=device)
        for prm in list(model.parameters()) + [b for b in model.buffers() if b.is_floating_point()]:
            prm.data = prm.data.to(dtype)
        return model.eval()
    return model.to(device=device, dtype=dtype).eval()


@torch.no_grad()
def calibrate_thresholds(model: Transformer, sparsities: Dict[str, List[float]], n_tokens: int = 24,
                         seed: int = 4321) -> List[Dict[str, float]]:
    """Synthetic mode: per layer and projection, tau = the `s` quantile of |activation| observed on a
    short dense run, so the kept fraction is 1 - s on the synthetic activations (the calibration
    histograms only describe real checkpoints).  Activation sites as in the reference:
    q/k/v <- attention input, o <- attention output, gate/up <- MLP input, down <- silu(g)*u."""
    if all(float(v) <= 0 for vals in sparsities.values() for v in vals):
        return [{p: -1.0 for p in PROJS} for _ in model.layers]
    dev = model.output.weight.device
    acts: List[Dict[str, List[torch.Tensor]]] = [dict(attn_in=[], attn_out=[], mlp_in=[], mlp_mid=[]) for _ in model.layers]
    hooks = []
    for i, layer in enumerate(model.layers):
        hooks.append(layer.attention.register_forward_pre_hook(lambda m, a, i=i: acts[i]["attn_in"].append(a[0].detach().float().flatten())))
        hooks.append(layer.attention.wo.register_forward_pre_hook(lambda m, a, i=i: acts[i]["attn_out"].append(a[0].detach().float().flatten())))
        hooks.append(layer.feed_forward.register_forward_pre_hook(lambda m, a, i=i: acts[i]["mlp_in"].append(a[0].detach().float().flatten())))
        hooks.append(layer.feed_forward.w2.register_forward_pre_hook(lambda m, a, i=i: acts[i]["mlp_mid"].append(a[0].detach().float().flatten())))
    g = torch.Generator(device=dev).manual_seed(seed)
    toks = torch.randint(0, model.config.vocab_size, (n_tokens,), device=dev, generator=g, dtype=torch.int)
    model.setup_caches(max_batch_size=1, max_seq_length=max(n_tokens, 8))
    model(toks.view(1, -1), torch.arange(n_tokens, device=dev))  # one dense prefill = n_tokens activation samples
    for h in hooks:
        h.remove()
    site = {"q": "attn_in", "k": "attn_in", "v": "attn_in", "o": "attn_out", "gate": "mlp_in", "up": "mlp_in", "down": "mlp_mid"}
    out = []
    for i in range(len(model.layers)):
        th = {}
        for p in PROJS:
            s = float(sparsities[p][i])
            if s <= 0:
                th[p] = -1.0  # keep everything (|x| > -1): the dense comparator on the same kernels
                continue
            a = torch.cat(acts[i][site[p]]).abs()
            th[p] = float(torch.quantile(a[:: max(1, a.numel() // 200000)], s))
        out.append(th)
    # the caches were sized for calibration; let generate() size them again
    model.max_seq_length = -1
    model.max_batch_size = -1
    return out


@torch.no_grad()
def refine_thresholds_on_decode(model: Transformer, sparsities: Dict[str, List[float]], ths: List[Dict[str, float]],
                                n_prompt: int = 24, n_decode: int = 200) -> List[Dict[str, float]]:
    """Synthetic mode, GPU: re-take the thresholds on the DECODE path (engine.calibrate_on_decode) so that every
    projection keeps its target fraction on decode activations — with random weights the attention output shrinks with
    the context length, and thresholds from a short prefill keep ~10 % of the o-projection's rows after 100 positions.
    The refined values are written back into the blocks' thresh_* attributes; the caches are released again."""
    dev = model.output.weight.device
    span = min(n_decode, model.config.block_size - n_prompt - 8)
    if span < 8:
        return ths
    model.max_seq_length, model.max_batch_size = -1, -1
    model.setup_caches(max_batch_size=1, max_seq_length=n_prompt + span + 8)
    from teal_amd.gpt_fast.engine import pick_engine
    cls, _why = pick_engine(model)
    if cls is None:  # e.g. head_dim 48: the module path decodes it, with the prefill thresholds
        model.max_seq_length, model.max_batch_size = -1, -1
        return ths
    toks = torch.randint(0, model.config.vocab_size, (n_prompt,), device=dev, dtype=torch.int,
                         generator=torch.Generator(device=dev).manual_seed(97))
    model(toks.view(1, -1), torch.arange(n_prompt, device=dev))
    eng = cls(model, ths)
    ths = eng.calibrate_on_decode(sparsities, toks[-1:].clone(), n_prompt, span)
    from teal_amd.gpt_fast import tp
    ths = tp.sync_thresholds(ths, model)
    for layer, th in zip(model.layers, ths):
        at, ff = layer.attention, layer.feed_forward
        at.thresh_q, at.thresh_k, at.thresh_v, at.thresh_o = th["q"], th["k"], th["v"], th["o"]
        ff.thresh_gate, ff.thresh_up, ff.thresh_down = th["gate"], th["up"], th["down"]
    del eng
    model.max_seq_length, model.max_batch_size = -1, -1  # let generate() size the caches again
    return ths


def apply_sparsity(model: Transformer, *, sparsity: float, hist_path: Optional[str], greedy_lookup: Optional[str],
                   synthetic: bool, decode_calibration: bool = True) -> List[Dict[str, float]]:
    """monkeypatch every layer (gpt-fast/generate.py:328-331); returns the thresholds used."""
    L = len(model.layers)
    if greedy_lookup and greedy_lookup.endswith(".json"):
        # block-wise greedy table captured from the reference (tests/golden/greedy_*.json, generated by
        # oracle/gen_golden.py from models/<name>/lookup): {"targets": {"0.5": {"sparsities": {proj: [...]}}}}
        with open(greedy_lookup) as f:
            table = json.load(f)["targets"][repr(float(sparsity))]["sparsities"]
        sparsities = {p: [float(v) for v in table[p][:L]] for p in PROJS}
        assert all(len(v) == L for v in sparsities.values()), "greedy table has fewer layers than the model"
    elif greedy_lookup:
        sparsities = get_layer_greedy_sparsities([sparsity] * L, greedy_lookup)
    else:
        sparsities = {p: [sparsity] * L for p in PROJS}
    device = model.output.weight.device.type
    if synthetic or hist_path is None:
        from teal_amd.gpt_fast import tp
        ths = tp.sync_thresholds(calibrate_thresholds(model, sparsities), model)  # (one tau per site on every rank; no-op without TP)
        for i, layer in enumerate(model.layers):
            monkeypatch_layer(i, layer, sparsity, None, device, thresholds=ths[i])
        if decode_calibration and device == "cuda" and any(float(v) > 0 for vals in sparsities.values() for v in vals):
            ths = refine_thresholds_on_decode(model, sparsities, ths)
    else:
        ths = [monkeypatch_layer(i, layer, sparsity, hist_path, device, sparsities=sparsities)
               for i, layer in enumerate(model.layers)]
    return ths


@torch.no_grad()
def report_kept_fractions(model: Transformer, thresholds, prompt: torch.Tensor) -> Dict[str, float]:
    """Achieved kept fraction per projection (the quantity that determines the bytes read), measured on
    one pass of the prompt through the patched model with the installed thresholds."""
    acts = {k: [] for k in ("attn_in", "attn_out", "mlp_in", "mlp_mid")}
    site = {"q": "attn_in", "k": "attn_in", "v": "attn_in", "o": "attn_out", "gate": "mlp_in", "up": "mlp_in", "down": "mlp_mid"}
    kept = {p: [] for p in PROJS}
    hooks = []
    for i, layer in enumerate(model.layers):
        th = thresholds[i]

        def pre_attn(m, a, th=th):
            x = a[0].detach().float().abs()
            for p in ("q", "k", "v"):
                kept[p].append(float((x > th[p]).float().mean()))

        def pre_ffn(m, a, th=th):
            x = a[0].detach().float().abs()
            for p in ("gate", "up"):
                kept[p].append(float((x > th[p]).float().mean()))

        hooks.append(layer.attention.register_forward_pre_hook(pre_attn))
        hooks.append(layer.feed_forward.register_forward_pre_hook(pre_ffn))
    model(prompt.view(1, -1), torch.arange(prompt.numel(), device=prompt.device))
    for h in hooks:
        h.remove()
    out = {p: sum(v) / len(v) for p, v in kept.items() if v}
    print("achieved kept fraction (prompt activations):", {k: round(v, 3) for k, v in out.items()})
    return out


def _get_model_size(model) -> int:
    size = 0
    for _, child in model.named_children():
        if not isinstance(child, torch.nn.Embedding):
            size += sum(p.numel() * p.dtype.itemsize for p in itertools.chain(child.parameters(), child.buffers()))
    return size


# ------------------------------------------------------------------------------------------------
# decode step + hipGraph capture
# ------------------------------------------------------------------------------------------------
class GraphedDecoder:
    """decode_one_token (gpt-fast/generate.py:73-77) with static buffers, captured once into a hipGraph
    (the reference gets the same effect from torch.compile(mode="reduce-overhead"), generate.py:420)."""

    def __init__(self, model: Transformer, use_graph: bool, temperature: float, top_k: Optional[int]):
        self.model, self.use_graph = model, use_graph
        self.kw = dict(temperature=temperature, top_k=top_k)
        dev = model.device if hasattr(model, "device") else model.output.weight.device
        self.tok = torch.zeros(1, 1, dtype=torch.int, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.out_tok = None

    def _step(self):
        logits = self.model(self.tok, self.pos)
        if hasattr(self.model, "sample_fused"):  # HIP engine: one-launch sampler
            return self.model.sample_fused(logits, **self.kw)
        return sample(logits, **self.kw)[0]

    def capture(self, cur_token: Optional[torch.Tensor] = None, input_pos: Optional[torch.Tensor] = None):
        """cur_token / input_pos: where decoding stands.  The two eager warm-up steps and the capture run write the KV
        row of `input_pos` (rewritten with the same values by the first replay) — without them they would run at the
        stale buffers' position (0 after construction) and overwrite the first prompt token's K/V."""
        if not self.use_graph or self.graph is not None:
            return
        if cur_token is not None:
            self.tok.copy_(cur_token.view(1, 1))
        if input_pos is not None:
            self.pos.copy_(input_pos)
        self.graph, self.out_tok = runtime.capture_graph(self._step, warmups=2)  # (warm-ups: workspace + allocator pools)

    def __call__(self, cur_token: torch.Tensor, input_pos: torch.Tensor) -> torch.Tensor:
        self.tok.copy_(cur_token.view(1, 1))
        self.pos.copy_(input_pos)
        if self.graph is not None:
            self.graph.replay()
            return self.out_tok
        return self._step()


class GraphedPrefill:
    """`--compile_prefill` (gpt-fast/generate.py:423-425, 540): the prompt pass captured into a hipGraph per prompt
    length (the reference compiles `prefill` with Inductor).  Static token / position buffers, kept alive with the
    graph; the model's KV caches must not be re-allocated between capture and replay (setup_caches keeps them
    when the sizes are unchanged; a new cache object gets a new graph)."""

    MAX_GRAPHS = 4  # distinct (prompt length, buffers) keys kept; each graph owns a private memory pool (--interactive with
                    # varying prompt lengths would otherwise grow one per new length forever): least recently used goes first

    def __init__(self, model: Transformer):
        self.model = model
        self.graphs = collections.OrderedDict()
        self.eager_reason = None  # set when a capture failed under tensor parallelism: the pass then runs op by op

    def __call__(self, prompt: torch.Tensor) -> torch.Tensor:
        T = prompt.numel()
        if self.eager_reason is not None:
            return self.model(prompt.view(1, -1), torch.arange(0, T, device=prompt.device))
        # everything the captured launches hold raw pointers to: a re-laid-out weight (DecodeEngine / monkeypatch
        # to_column_major replace the storage) or a re-allocated KV cache forces a new capture
        key = (T,) + pointer_key(self.model, freqs=False)
        if key not in self.graphs:
            dev = prompt.device
            toks = torch.zeros(1, T, dtype=torch.int, device=dev)
            pos = torch.arange(0, T, device=dev)
            toks.copy_(prompt.view(1, -1))
            try:  # (the warm-up outside capture: allocator pools, GEMM heuristics)
                g, logits = runtime.capture_graph(lambda: self.model(toks, pos))
            except Exception as e:  # noqa: BLE001
                # a sharded model's pass holds one all-reduce per attention and per MLP (tp._reduce_hook): if the collective
                # cannot be captured on this stack, run the pass op by op instead of aborting the run (no silent change for an
                # unsharded model: there a capture failure is a bug and propagates)
                if int(getattr(self.model, "tp_world", 1)) < 2:
                    raise
                self.eager_reason = f"{type(e).__name__}: {e}"
                print(f"teal_amd: hipGraph capture of the tensor-parallel prompt pass failed ({self.eager_reason}); running it eagerly")
                torch.cuda.synchronize()
                return self.model(prompt.view(1, -1), torch.arange(0, T, device=dev))
            self.graphs[key] = (g, toks, pos, logits)  # every tensor the graph reads or writes stays alive
            while len(self.graphs) > self.MAX_GRAPHS:
                torch.cuda.synchronize()  # the evicted graph's pool goes back to the allocator: nothing of it may be in flight
                self.graphs.popitem(last=False)
        self.graphs.move_to_end(key)
        g, toks, _pos, logits = self.graphs[key]
        toks.copy_(prompt.view(1, -1))
        g.replay()
        return logits


class EngineDecoder:
    """GraphedDecoder's role for the fused HIP engine: built lazily once the KV caches exist."""

    def __init__(self, torch_model: Transformer, thresholds, use_graph: bool, temperature: float, top_k: Optional[int]):
        self.torch_model, self.thresholds, self.use_graph = torch_model, thresholds, use_graph
        self.kw = dict(temperature=temperature, top_k=top_k)
        self._engine, self._key = None, None

    def _cache_key(self):
        return pointer_key(self.torch_model, weights=False)

    @property
    def model(self):
        # the engine's launch descriptors hold the KV caches' raw pointers: rebuild when setup_caches re-allocated them
        # (same size or not), not only when the context length changed
        key = self._cache_key()
        if self._engine is None or self._key != key:
            from teal_amd.gpt_fast.engine import pick_engine
            cls, why = pick_engine(self.torch_model)
            if cls is None:
                raise ValueError(f"no fused engine for this model: {why}")
            self._engine, self._key = cls(self.torch_model, self.thresholds), key
        return self._engine


def relayout_for_engine(model: Transformer) -> None:
    """The fused engine re-lays every projection (and lm_head) out column-major when it is built — lazily, after the first
    prefill.  Do it up front so that a prefill graph never captures pointers to storage that is freed later."""
    relayout(model)


@torch.no_grad()
def generate(model: Transformer, prompt: torch.Tensor, max_new_tokens: int, decoder: GraphedDecoder,
             temperature: float = 0.8, top_k: Optional[int] = 200, prefill: Optional[GraphedPrefill] = None,
             processors: Optional[Dict] = None, sampling: Optional[Dict] = None) -> torch.Tensor:
    """prefill (seq > 1: ops fall back to dense matmul) then max_new_tokens-1 decode steps.  processors (the fused engine only):
    repetition_penalty / presence_penalty / frequency_penalty / logit_bias of this sample, applied to every draw.  sampling (the
    fused engine only): top_p / min_p of this sample, next to the decoder's temperature and top_k, for every draw."""
    T = prompt.size(0)
    T_new = T + max_new_tokens
    dev = prompt.device
    model.setup_caches(max_batch_size=1, max_seq_length=min(T_new, model.config.block_size))
    seq = torch.empty(T_new, dtype=prompt.dtype, device=dev)
    seq[:T] = prompt
    logits = prefill(prompt) if prefill is not None else model(prompt.view(1, -1), torch.arange(0, T, device=dev))
    eng = decoder.model if hasattr(decoder.model, "decode_n") else None
    if processors:
        if eng is None or logits.dtype != eng.dtype or logits.shape[-1] != eng.cfg.vocab_size:
            raise ValueError("logit processors need the fused engine's sampler for every draw")
        if eng.adj_logits is None:
            eng.set_logit_processors(True)
        eng.set_slot_processors(0, prompt.tolist(), **processors)
    if sampling:
        if eng is None or logits.dtype != eng.dtype or logits.shape[-1] != eng.cfg.vocab_size:
            raise ValueError("top_p / min_p need the fused engine's sampler for every draw")
        if eng.sampling_params is None:
            eng.set_sampling_params(True)
        eng.set_slot_sampling(0, decoder.kw["temperature"], decoder.kw["top_k"], **sampling)
    if eng is not None and logits.dtype == eng.dtype and logits.shape[-1] == eng.cfg.vocab_size:
        # HIP engine: the token after the prompt comes from the same fused sampler as every later one (gpt-fast/generate.py:
        # 49-66 is ONE function for both), and the whole loop stays on the device
        next_token = eng.sample_first(logits[0, -1], decoder.kw["temperature"], decoder.kw["top_k"])
        seq[T] = next_token.view(())
        toks = eng.decode_n(next_token, T, max_new_tokens - 1, temperature=decoder.kw["temperature"],
                            top_k=decoder.kw["top_k"], use_graph=decoder.use_graph, drawn=1)
        seq[T + 1:] = toks.to(seq.dtype)
        return seq
    next_token = sample(logits, temperature=temperature, top_k=top_k)[0].clone()
    seq[T] = next_token
    if eng is not None:
        toks = eng.decode_n(next_token, T, max_new_tokens - 1, temperature=decoder.kw["temperature"],
                            top_k=decoder.kw["top_k"], use_graph=decoder.use_graph)
        seq[T + 1:] = toks.to(seq.dtype)
        return seq
    input_pos = torch.tensor([T], device=dev, dtype=torch.int)
    cur = next_token.view(1, -1)
    decoder.capture(cur, input_pos)
    for i in range(max_new_tokens - 1):
        nxt = decoder(cur, input_pos)
        input_pos += 1
        seq[T + 1 + i] = nxt.view(())
        cur = nxt.view(1, -1)
    return seq


# ------------------------------------------------------------------------------------------------
# speculative decoding (gpt-fast/generate.py:98-217, 392-398, 500-524): a TEAL-sparse draft, the dense model verifies
# ------------------------------------------------------------------------------------------------
def check_speculative_args(args) -> Optional[str]:
    """None (no speculation), "self" (the target's own weights draft, with TEAL thresholds) or "draft" (a separate checkpoint).
    Every refusal is raised here, before anything is loaded."""
    draft = getattr(args, "draft_checkpoint_path", None)
    self_spec = bool(getattr(args, "self_speculate", False))
    if draft is None and not self_spec:
        return None
    from teal_amd.gpt_fast.speculative import MAX_K
    k = int(getattr(args, "speculate_k", 5))
    if not 1 <= k <= MAX_K:
        raise SystemExit(f"speculative decoding: --speculate_k must be in 1..{MAX_K} (k + 1 tokens per verify pass), got {k}")
    if int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) > 1:
        raise SystemExit("speculative decoding does not run under tensor parallelism")
    if args.precision not in ("fp16", "bf16"):
        raise SystemExit(f"speculative decoding needs a 16-bit target, got --precision {args.precision}")
    if self_spec and draft is not None:
        raise SystemExit("speculative decoding: give --self_speculate or --draft_checkpoint_path, not both")
    if self_spec:
        if not args.synthetic:
            raise SystemExit("speculative decoding: --self_speculate is for --synthetic runs; with a checkpoint, pass it as "
                             "--draft_checkpoint_path too")
        return "self"
    if args.synthetic:
        raise SystemExit("speculative decoding: --synthetic runs self-speculate (--self_speculate); a draft checkpoint needs a target checkpoint")
    target = Path(args.checkpoint_path)
    if "int8" in str(target) or "int4" in str(target):  # (the loader's own test: load_checkpoint_model)
        raise SystemExit(f"speculative decoding verifies with a dense 16-bit target; {target} is quantised")
    draft = Path(draft)
    if not draft.is_file():
        raise SystemExit(f"speculative decoding: draft checkpoint {draft} not found")
    if draft.resolve() == target.resolve():
        return "self"
    try:
        vt, vd = ModelArgs.from_name(target.parent.name).vocab_size, ModelArgs.from_name(draft.parent.name).vocab_size
    except KeyError as e:
        raise SystemExit(f"speculative decoding: cannot tell the vocabulary of a checkpoint ({e})")
    if vt != vd:
        raise SystemExit(f"speculative decoding: the draft's vocabulary ({vd}) differs from the target's ({vt})")
    return "draft"


@torch.no_grad()
def speculative_generate(spec, prompt: torch.Tensor, max_new_tokens: int, prefill, draft_prefill=None,
                         temperature: float = 0.8, top_k: Optional[int] = 200):
    """prompt pass (target; the draft's too for a separate draft), the first token from the target's prompt logits, then rounds
    until max_new_tokens tokens are out (the last round's overshoot is trimmed).  Returns (sequence, accepted-count histogram)."""
    T = prompt.size(0)
    seq = torch.empty(T + max_new_tokens, dtype=prompt.dtype, device=prompt.device)
    seq[:T] = prompt
    logits = prefill(prompt)
    if draft_prefill is not None:
        draft_prefill(prompt)
    eng = spec.draft
    first = eng.sample_first(logits[0, -1].contiguous(), temperature, top_k)
    seq[T] = first.view(())
    if max_new_tokens > 1:
        seq[T + 1:] = spec.decode(first, T, max_new_tokens - 1).to(seq.dtype)
    return seq, spec.histogram()


def load_draft_model(path: Path, device: str, dtype: torch.dtype, sparsity: float, hist_path: Optional[str],
                     greedy_lookup: Optional[str]):
    """(draft model, its TEAL thresholds) from a checkpoint (16-bit, int8 or int4, as load_checkpoint_model reads it).  Sparsity 0
    without histograms: thresholds of -1 (every activation kept, a dense draft — calibrate_thresholds' convention)."""
    draft = load_checkpoint_model(Path(path), device, dtype)
    if hist_path is None and sparsity <= 0:
        return draft, [{p: -1.0 for p in PROJS} for _ in draft.layers]
    return draft, apply_sparsity(draft, sparsity=sparsity, hist_path=hist_path, greedy_lookup=greedy_lookup, synthetic=hist_path is None)


def build_speculator(model: Transformer, thresholds, k: int, temperature: float, top_k: Optional[int], capacity: int, max_seq: int,
                     use_graph: bool, draft=None):
    """(SpeculativeDecoder, draft prompt pass or None) for a target whose caches are set up (max_seq rows).  draft: None
    (self-speculation: the target's own weights with `thresholds` draft) or (draft model, its thresholds): a separate draft with
    its own caches, prompt pass and fill-in step."""
    from teal_amd.gpt_fast.engine import pick_engine
    from teal_amd.gpt_fast.prefill import FusedPrefill
    from teal_amd.gpt_fast.speculative import SpeculativeDecoder, VerifyPass
    why = VerifyPass.supports(model)
    if why is not None:
        raise SystemExit(f"speculative decoding cannot verify with this target: {why}")
    verify = VerifyPass(model)
    if draft is None:
        draft_model, draft_prefill = model, None
    else:
        draft_model, thresholds = draft
        if draft_model.config.vocab_size != model.config.vocab_size:
            raise SystemExit("speculative decoding: the draft's vocabulary differs from the target's")
        draft_model.setup_caches(max_batch_size=1, max_seq_length=max_seq)
        relayout_for_engine(draft_model)
        draft_prefill = FusedPrefill(draft_model, graph=use_graph)
    cls, why = pick_engine(draft_model)
    if cls is None:
        raise SystemExit(f"speculative decoding: no fused engine for the draft: {why}")
    eng = cls(draft_model, thresholds)
    spec = SpeculativeDecoder(eng, verify, k, temperature, top_k, fill_in=draft is not None, capacity=capacity, graph=use_graph)
    return spec, draft_prefill


def run_speculative(args, model: Transformer, thresholds, prompt: torch.Tensor, tokenizer, mode: str, device: str,
                    dtype: torch.dtype) -> Dict:
    """main()'s loop for speculative decoding: caches sized T_new + k + 1 (gpt-fast/generate.py:174), tokens/sec as the reference
    counts it (new tokens over the whole generate() call), and its acceptance printout (:500-524)."""
    from teal_amd.gpt_fast.prefill import FusedPrefill
    from teal_amd.gpt_fast.speculative import SpeculativeDecoder
    if mode == "self" and thresholds is None:
        raise SystemExit("speculative decoding needs TEAL thresholds for the draft (--hist_path, or --synthetic)")
    use_graph = bool(args.compile)
    T = prompt.numel()
    max_seq = min(T + args.max_new_tokens + args.speculate_k + 1, model.config.block_size)
    model.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    relayout_for_engine(model)
    prefill = FusedPrefill(model, graph=use_graph)
    draft = None
    if mode == "draft":
        draft = load_draft_model(Path(args.draft_checkpoint_path), device, dtype, args.sparsity, args.hist_path, args.greedy_lookup)
    spec, draft_prefill = build_speculator(model, thresholds, args.speculate_k, args.temperature, args.top_k,
                                           args.max_new_tokens + args.speculate_k + 1, max_seq, use_graph, draft)
    model_size = _get_model_size(model)
    tps, seqs, hist = [], [], [0] * (args.speculate_k + 1)
    for i in range(-1 if args.compile else 0, args.num_samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y, h = speculative_generate(spec, prompt, args.max_new_tokens, prefill, draft_prefill, args.temperature, args.top_k)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if i == -1:
            print(f"Graph capture + warm-up time: {t:.2f} seconds")
            continue
        hist = [a + b for a, b in zip(hist, h)]
        tps.append((y.size(0) - T) / t)
        seqs.append(y.tolist())
        if tokenizer is not None:
            print(tokenizer.decode(y.tolist()))
        print(f"Time for inference {i + 1}: {t:.02f} sec total, {tps[-1]:.02f} tokens/sec")
        print(f"Bandwidth achieved: {model_size * tps[-1] / 1e9:.02f} GB/s (dense parameter bytes x tok/s, as the reference reports)")
    print("==========")
    st = SpeculativeDecoder.acceptance_stats(hist)
    print(f"Acceptance probs: {st['acceptance_probs']}")
    print(f"Mean Accepted: {st['mean_accepted']}")
    mean = sum(tps) / max(1, len(tps))
    print(f"Average tokens/sec: {mean:.2f}")
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB")
    return {"tokens_per_sec": tps, "mean_tokens_per_sec": mean, "thresholds": thresholds, "decoder": "SpeculativeDecoder",
            "sequences": seqs, "prefill": "FusedPrefill", "speculative": mode, "acceptance_histogram": hist,
            "acceptance_probs": st["acceptance_probs"], "mean_accepted": st["mean_accepted"]}


# ------------------------------------------------------------------------------------------------
# ------------------------------------------------------------------------------------------------
# batched decode (--batch_size B): B sequences per step, each TEAL-masked by its own activations
# ------------------------------------------------------------------------------------------------
def check_batched_args(args) -> int:
    """the batch size; every refusal is raised here, before anything is loaded"""
    from teal_amd.kernels.sparse_gemv import BATCH_MAX
    B = int(getattr(args, "batch_size", 1) or 1)
    if B == 1:
        return 1
    if not 1 <= B <= BATCH_MAX:
        raise SystemExit(f"batched decode: --batch_size must be in 1..{BATCH_MAX}, got {B}")
    if getattr(args, "draft_checkpoint_path", None) is not None or getattr(args, "self_speculate", False):
        raise SystemExit("batched decode does not combine with speculative decoding")
    if int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) > 1:
        raise SystemExit("batched decode does not run under tensor parallelism")
    if getattr(args, "interactive", False):
        raise SystemExit("batched decode does not combine with --interactive")
    if args.precision not in ("fp16", "bf16") or (not args.synthetic and ("int8" in str(args.checkpoint_path) or "int4" in str(args.checkpoint_path))):
        raise SystemExit("batched decode needs 16-bit weights (int8 / int4 checkpoints decode one sequence at a time)")
    return B


def _engine_path_refusals(args, flags: str, plural: bool, why_spec: str, why_engine: str) -> None:
    """the four refusals every feature that lives in a launch of the fused engines' step shares: speculative decoding, tensor
    parallelism, no TEAL thresholds, no engine path.  flags: as the user wrote them (plural: more than one); why_spec /
    why_engine: the feature's own reason behind the first ("" for none) and the last"""
    do, need = ("do", "need") if plural else ("does", "needs")
    if getattr(args, "draft_checkpoint_path", None) is not None or getattr(args, "self_speculate", False):
        raise SystemExit(f"{flags} {do} not combine with speculative decoding{why_spec}")
    if int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) > 1:
        raise SystemExit(f"{flags} {do} not run under tensor parallelism (a rank's lm_head holds a slice of the vocabulary)")
    if getattr(args, "dense", False) or (not args.synthetic and args.hist_path is None):
        raise SystemExit(f"{flags} {need} TEAL thresholds (--hist_path, or --synthetic): the fused engines run patched models only")
    if getattr(args, "requests", None) is None and (getattr(args, "no_engine", False) or not (args.compile or args.engine)):
        raise SystemExit(f"{flags} {need} a fused engine (--compile or --engine, without --no_engine, or --requests): the module "
                         f"path{why_engine}")


def check_logprobs_args(args) -> Optional[int]:
    """--logprobs: None (off), 0 (each generated token's logprob) or 1..8 (and that many most likely alternates); every refusal
    is raised here, before anything is loaded.  The logprobs come from a launch inside the fused engines' step, so the flag
    needs an engine path: --compile / --engine (one sequence or --batch_size) or --requests."""
    n = getattr(args, "logprobs", None)
    if n is None:
        return None
    if not 0 <= int(n) <= 8:
        raise SystemExit(f"--logprobs must be in 0..8 (alternates per token), got {n}")
    _engine_path_refusals(args, "--logprobs", False, "", " returns token ids only")
    return int(n)


def check_processor_args(args) -> Dict:
    """--repetition_penalty / --presence_penalty / --frequency_penalty: the controls that are switched on ({}: none); every
    refusal is raised here, before anything is loaded.  The processors are a launch in front of the fused engines' samplers, so
    the flags need an engine path: --compile / --engine (one sequence or --batch_size) or --requests, where they are the
    defaults of requests that carry none of their own."""
    from teal_amd.gpt_fast.continuous import parse_controls
    c = {}
    for name, rule in (("repetition_penalty", "a finite number > 0 (1: off)"), ("presence_penalty", "a finite number"),
                       ("frequency_penalty", "a finite number")):
        if getattr(args, name, None) is not None:
            try:
                c.update(parse_controls({name: getattr(args, name)}, "generate"))
            except ValueError:
                raise SystemExit(f"--{name} must be {rule}") from None
    c = {k: v for k, v in c.items() if v != (1.0 if k == "repetition_penalty" else 0.0)}
    if not c:
        return {}
    _engine_path_refusals(args, "--repetition_penalty / --presence_penalty / --frequency_penalty", True,
                          " (the accept rule compares the models' own distributions)", " samples from the raw logits")
    return c


def check_sampling_args(args) -> Dict:
    """--top_p / --min_p: {} when both are off, else {"top_p": ..., "min_p": ...}; every refusal is raised here, before anything is
    loaded.  Nucleus and min-p sampling live in the fused engines' per-request sampling launch, so the flags need an engine path:
    --compile / --engine (one sequence or --batch_size), where they are the setting of every row, or --requests, where they are
    the defaults of requests that carry none of their own."""
    from teal_amd.gpt_fast.sampling import check_sampling
    c = {"top_p": 1.0 if getattr(args, "top_p", None) is None else args.top_p, "min_p": 0.0 if getattr(args, "min_p", None) is None else args.min_p}
    for name, rule in (("top_p", "a finite number > 0 (1: off)"), ("min_p", "a number in [0, 1) (0: off)")):
        try:
            check_sampling(**{name: c[name]})
        except ValueError:
            raise SystemExit(f"--{name} must be {rule}, got {c[name]!r}") from None
    if c["top_p"] >= 1.0 and c["min_p"] == 0.0:
        return {}
    _engine_path_refusals(args, "--top_p / --min_p", True, " (the accept rule compares the models' distributions under one temperature "
                          "and top_k)", "'s sampler knows temperature and top_k only")
    return c


def check_stop_args(args) -> Dict:
    """--stop_token_ids / --min_new_tokens / --finish_reason: the batcher's keywords that are switched on ({}: none); every refusal
    is raised here, before anything is loaded.  Stop conditions live in the retire launch of continuous batching — no other
    engine retires — so the flags are valid with --requests only, where the first two are the defaults of requests that carry none
    of their own."""
    out = {}
    raw = getattr(args, "stop_token_ids", None)
    if raw is not None:
        try:
            ids = [int(x) for x in str(raw).split(",") if x.strip()]
        except ValueError:
            ids = None
        if not ids or any(t < 0 for t in ids) or len(set(ids)) > 16:
            raise SystemExit(f"--stop_token_ids must be 1..16 token ids (>= 0) separated by commas, got {raw!r}")
        out["stop_token_ids"] = ids
    n = getattr(args, "min_new_tokens", None)
    if n is not None:
        if int(n) < 0:
            raise SystemExit(f"--min_new_tokens must be >= 0, got {n}")
        if int(n) > 0:
            out["min_new_tokens"] = int(n)
    if getattr(args, "finish_reason", False):
        out["finish_reason"] = True
    if out and getattr(args, "requests", None) is None:
        raise SystemExit("--stop_token_ids / --min_new_tokens / --finish_reason need --requests: stop conditions live in the retire "
                         "launch of continuous batching, and no other decode path retires")
    return out


def check_kv_cache_args(args) -> Optional[str]:
    """--kv_cache: the engine's keyword (None: the model's 16-bit caches; "fp8"); refused here, before anything is loaded, anywhere
    but under --requests: the fp8 cache is filled at an admission, and only continuous batching admits"""
    fmt = getattr(args, "kv_cache", "model") or "model"
    if fmt != "model" and getattr(args, "requests", None) is None:
        raise SystemExit(f"--kv_cache {fmt} needs --requests: the fp8 KV cache is filled where a request is admitted (its prompt's rows "
                         "are quantised there), and no other decode path admits")
    return None if fmt == "model" else fmt


def _mean_logprob_line(lps) -> str:
    return f"    mean logprob {sum(lps) / max(1, len(lps)):.4f} over {len(lps)} tokens (model distribution, temperature 1)"


@torch.no_grad()
def run_batched(args, model: Transformer, thresholds, prompts: torch.Tensor, tokenizer, use_engine: bool) -> Dict:
    """prompts [B, T]: a dense prompt pass through the module path at batch B, then max_new_tokens - 1 steps through
    BatchedDecodeEngine (one hipGraph replay per step under --compile) or the patched ops at batch B"""
    B, T = prompts.shape
    dev = prompts.device
    n_new = args.max_new_tokens
    max_seq = min(T + n_new, model.config.block_size)
    n_new = max_seq - T
    model.setup_caches(max_batch_size=B, max_seq_length=max_seq)
    eng = None
    if use_engine:
        from teal_amd.gpt_fast.batched import BatchedDecodeEngine
        why = BatchedDecodeEngine.supports(model)
        if why is None:
            eng = BatchedDecodeEngine(model, thresholds, B)
        else:
            print(f"batched engine not used: {why}")
    n_lp = getattr(args, "logprobs", None)
    if n_lp is not None:
        if eng is None:
            raise SystemExit("--logprobs: the batched engine cannot run this model, and the module path returns token ids only")
        eng.set_logprobs(n_lp)
    proc = check_processor_args(args)
    if proc:  # the first token of each sequence comes from the prompt pass's torch sampler: the processors act from the second on
        if eng is None:
            raise SystemExit("logit processors: the batched engine cannot run this model, and the module path samples from the raw logits")
        eng.set_logit_processors(True)
        for b in range(B):
            eng.set_slot_processors(b, prompts[b].tolist(), **proc)
    samp = check_sampling_args(args)
    if samp:  # every draw under the flags: the first token of each sequence comes from the sampling launch too (sample_first)
        if eng is None:
            raise SystemExit("--top_p / --min_p: the batched engine cannot run this model, and the module path's sampler knows "
                             "temperature and top_k only")
        eng.set_sampling_params(True)
        for b in range(B):
            eng.set_slot_sampling(b, args.temperature, args.top_k, **samp)
    tps, seqs, lps, tops = [], [], [], []
    for i in range(-1 if args.compile else 0, args.num_samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = torch.empty(B, T + n_new, dtype=torch.int64, device=dev)
        seq[:, :T] = prompts
        logits = model(prompts.long(), torch.arange(0, T, device=dev))  # [B, T, V], dense (the ops' prefill path)
        if samp:
            eng.manual_seed(1234 + max(i, 0))
        first = eng.sample_first(logits[:, -1]).long() if samp else sample_batch(logits[:, -1], args.temperature, args.top_k)
        seq[:, T] = first
        if n_new > 1:
            if eng is not None:
                eng.manual_seed(1234 + max(i, 0))
                seq[:, T + 1:] = eng.decode_n(first, T, n_new - 1, args.temperature, args.top_k, use_graph=bool(args.compile),
                                              prompt_tokens=prompts.tolist() if proc else None).long()
            else:
                cur, pos = first.view(B, 1), torch.tensor([T], device=dev)
                for j in range(n_new - 1):
                    cur = sample_batch(model(cur, pos)[:, -1], args.temperature, args.top_k).view(B, 1)
                    seq[:, T + 1 + j] = cur.view(B)
                    pos += 1
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if i == -1:
            print(f"Graph capture + warm-up time: {t:.2f} seconds")
            continue
        tps.append(B * n_new / t)
        seqs.append(seq.tolist())
        if n_lp is not None:  # of the tokens the engine drew: seq[:, T + 1:] (the first comes from the prompt pass's torch sampler)
            lp, ids, tlp = eng.read_logprobs(n_new - 1)
            lps.append(lp.tolist())
            tops.append([[list(zip(a, b_)) for a, b_ in zip(ii, vv)] for ii, vv in zip(ids.tolist(), tlp.tolist())])
        for b in range(B):
            text = tokenizer.decode(seq[b].tolist()) if tokenizer is not None else seq[b, T:].tolist()
            print(f"[sample {i + 1}, sequence {b}] {text}")
            if n_lp is not None and tokenizer is not None:
                print(_mean_logprob_line(lps[-1][b]))
        print(f"Time for inference {i + 1}: {t:.02f} sec total, {tps[-1]:.02f} tokens/sec aggregate, "
              f"{tps[-1] / B:.02f} tokens/sec per sequence (batch {B})")
    print("==========")
    mean = sum(tps) / max(1, len(tps))
    print(f"Average tokens/sec: {mean:.2f} aggregate, {mean / B:.2f} per sequence")
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB")
    return {"tokens_per_sec": tps, "mean_tokens_per_sec": mean, "mean_tokens_per_sec_per_sequence": mean / B, "batch_size": B,
            "thresholds": thresholds, "decoder": type(eng).__name__ if eng is not None else "module", "sequences": seqs,
            **({"logprobs": lps, "logprob_offset": T + 1} if n_lp is not None else {}),
            **({"top_logprobs": tops} if n_lp else {})}


# ------------------------------------------------------------------------------------------------
# continuous batching (--requests FILE): requests of any prompt length and budget share the --batch_size slots
# ------------------------------------------------------------------------------------------------
def check_requests_args(args) -> int:
    """the number of slots; every refusal of batched decode and those of continuous batching, before anything is loaded"""
    ns = argparse.Namespace(**vars(args))
    ns.batch_size = max(2, int(getattr(args, "batch_size", 1) or 1))  # (batch 1 is served as one slot: the same refusals apply)
    check_batched_args(ns)
    if getattr(args, "no_engine", False):
        raise SystemExit("--requests runs through the batched HIP engine: it does not combine with --no_engine")
    if getattr(args, "no_fused_decode", False):
        raise SystemExit("--requests runs through the fused batched step: it does not combine with --no_fused_decode")
    if getattr(args, "dense", False) or (not args.synthetic and args.hist_path is None):
        raise SystemExit("--requests needs TEAL thresholds (--hist_path, or --synthetic): the batched engine runs patched models only")
    if int(getattr(args, "sync_every", 8)) < 1:
        raise SystemExit("--sync_every must be >= 1")
    if getattr(args, "eos_id", None) is not None and args.eos_id < 0:
        raise SystemExit("--eos_id must be a token id (>= 0)")
    return int(getattr(args, "batch_size", 1) or 1)


def _read_lines(path) -> List[str]:
    return Path(path).read_text().splitlines()


def check_request_files(args):
    """--requests, --prefixes and --constraints, each read once -> (request lines, prefix lines, the constraints parsed, the
    requests' sparsity levels).  What needs neither the model nor a tokenizer is refused here, before anything is loaded, in this
    order: a malformed automaton or a request on a constraint nobody defined, a request on a prefix nobody defined, a malformed
    "forced_tokens" / "forced_text" field (or one on a prefix line, or a "forced_text" under --synthetic), and
    check_request_sparsity's refusals"""
    from teal_amd.gpt_fast.continuous import check_constraint_ids, check_forced_fields, check_prefix_ids, parse_constraints
    cf, pf = getattr(args, "constraints", None), getattr(args, "prefixes", None)
    try:
        request_lines = _read_lines(args.requests)
        constraints = parse_constraints(_read_lines(cf)) if cf is not None else {}
        check_constraint_ids(request_lines, constraints)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--constraints: {e}" if cf is not None else f"--requests: {e}")
    try:
        prefix_lines = _read_lines(pf) if pf is not None else []
        check_prefix_ids(request_lines, prefix_lines)
        check_forced_fields(request_lines, prefix_lines, tokenizer_expected=not getattr(args, "synthetic", None))
    except (OSError, ValueError) as e:
        raise SystemExit(f"--requests: {e}")
    return request_lines, prefix_lines, constraints, check_request_sparsity(args, request_lines)


def check_request_sparsity(args, request_lines: Optional[List[str]] = None) -> List[float]:
    """the distinct "sparsity" levels the --requests lines carry (request_lines: the file's, where the caller has read it),
    ascending; every refusal is raised here, before anything is loaded: a level outside [0, 1), more than 8 distinct levels, and a
    level the run's threshold source cannot serve (a --greedy_lookup .json table holds its own list of targets; histograms and
    --synthetic calibration serve any level)"""
    from teal_amd.gpt_fast.continuous import check_sparsity_fields
    servable = None
    lookup = getattr(args, "greedy_lookup", None)
    if lookup and str(lookup).endswith(".json"):
        with open(lookup) as f:
            targets = set(json.load(f)["targets"])

        def servable(level):
            if level == 0.0 or repr(float(level)) in targets:
                return None
            return f"--greedy_lookup {lookup} has no such target (it holds {', '.join(sorted(targets))})"
    try:
        return check_sparsity_fields(_read_lines(args.requests) if request_lines is None else request_lines, servable)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--requests: {e}")


def resolve_sparsity_levels(args, model: Transformer, levels) -> Dict[float, List[Dict[str, float]]]:
    """each level -> its per-layer thresholds, through apply_sparsity — the function that resolves --sparsity — on the model's
    dense forward (a level is what a run at that --sparsity would use); level 0 keeps every row.  The caller patches the model at
    the run's own level afterwards."""
    out = {}
    for level in levels:
        if level == 0.0:
            continue
        for layer in model.layers:  # back to the dense forward: calibration must not see the last level's masks
            for m in (layer.attention, layer.feed_forward):
                m.__dict__.pop("forward", None)
        out[level] = apply_sparsity(model, sparsity=level, hist_path=args.hist_path, greedy_lookup=args.greedy_lookup,
                                    synthetic=bool(args.synthetic))
    if out:
        for layer in model.layers:
            for m in (layer.attention, layer.feed_forward):
                m.__dict__.pop("forward", None)
    if 0.0 in levels:
        out[0.0] = None  # (filled in by the caller from the run's thresholds: dense_thresholds needs their keys)
    return out


@torch.no_grad()
def run_continuous(args, model: Transformer, thresholds, tokenizer, request_lines, prefix_lines=(), constraints=None,
                   sparsity_levels=None) -> Dict:
    """--requests FILE through ContinuousBatcher on a SlotDecodeEngine of --batch_size slots (one hipGraph replay per step under
    --compile, with one warm-up run first).  request_lines / prefix_lines / constraints: what check_request_files read"""
    from teal_amd.gpt_fast.batched import SlotDecodeEngine
    from teal_amd.gpt_fast.continuous import ContinuousBatcher, cache_rows, parse_prefixes, parse_requests
    from teal_amd.gpt_fast.forcing import check_forced
    from teal_amd.gpt_fast.stopping import check_stops
    B = int(args.batch_size)
    constraints = constraints or {}
    for name, a in constraints.items():  # a token outside this model's vocabulary: refused before anything runs
        try:
            a.check(model.config.vocab_size, args.eos_id, eos_known=args.eos_id is not None)
        except ValueError as e:
            raise SystemExit(f"--constraints: constraint {name!r}: {e}")
    try:
        prefixes = parse_prefixes(prefix_lines, tokenizer)
    except ValueError as e:
        raise SystemExit(f"--prefixes: {e}")
    stop_kw = check_stop_args(args)
    try:
        reqs = parse_requests(request_lines, args.max_new_tokens, tokenizer, args.eos_id, prefixes=prefixes, constraints=constraints)
        max_seq = cache_rows(reqs, model.config.block_size, prefixes)
        if prefixes:  # (a prefix no request names is registered too: it needs room for a one-token suffix)
            max_seq = max(max_seq, min(max(len(t) for t in prefixes.values()) + 2, model.config.block_size))
        for i, r in enumerate(reqs):  # an id outside this model's vocabulary: refused before anything runs
            try:
                check_forced(model.config.vocab_size, r.forced_tokens)
                check_stops(model.config.vocab_size, **r.stops(stop_kw))
            except ValueError as e:
                raise ValueError(f"request {i}: {e}") from None
    except ValueError as e:
        raise SystemExit(f"--requests: {e}")
    kv_cache = check_kv_cache_args(args)
    # (fp8: the model's caches are the staging cache of the prompt passes, one sequence; the engine owns the slots' rows)
    model.setup_caches(max_batch_size=B if kv_cache is None else 1, max_seq_length=max_seq)
    why = SlotDecodeEngine.supports(model, kv_cache=kv_cache)
    if why is not None:
        raise SystemExit(f"--requests: the batched engine cannot run this model: {why}")
    eng = SlotDecodeEngine(model, thresholds, B, kv_cache=kv_cache)
    kvb = eng.kv_cache_bytes()
    print(f"KV cache ({'model' if kv_cache is None else kv_cache}): {kvb['staging'] / 1e6:.2f} MB 16-bit "
          f"({'the slots' if kv_cache is None else 'the staging cache'}), {kvb['codes'] / 1e6:.2f} MB codes, {kvb['scales'] / 1e6:.2f} MB scales")
    batcher = ContinuousBatcher(eng, sync_every=args.sync_every, temperature=args.temperature, top_k=args.top_k, seed=1234,
                                use_graph=bool(args.compile), prefixes=prefixes, logprobs=getattr(args, "logprobs", None),
                                **check_processor_args(args), **check_sampling_args(args), **stop_kw,
                                **({"constraints": constraints} if constraints else {}),
                                sparsity=float(args.sparsity), sparsity_levels=sparsity_levels or {})
    try:
        for name, toks in prefixes.items():  # once, before the warm-up run
            eng.register_prefix(name, toks)
    except ValueError as e:
        raise SystemExit(f"--prefixes: {e}")
    if prefixes:
        print(f"{len(prefixes)} shared prefixes registered: {eng.prefix_bytes() / 1e6:.2f} MB of K / V rows kept on the device")
    if args.compile:
        t0 = time.perf_counter()
        batcher.run(reqs)
        eng.reset_stats()
        print(f"Graph capture + warm-up time: {time.perf_counter() - t0:.2f} seconds")
    res = batcher.run(reqs)
    for i, toks in enumerate(res["tokens"]):
        text = tokenizer.decode(prefixes.get(reqs[i].prefix, []) + reqs[i].tokens + toks) if tokenizer is not None else toks
        print(f"[request {i}, slot {res['slots'][i]}] {text}")
        if "logprobs" in res and tokenizer is not None:
            print(_mean_logprob_line(res["logprobs"][i]))
        if res.get("forced", [None] * len(reqs))[i] is not None:
            print(f"    {res['forced'][i]} forced tokens: loglikelihood {res['loglikelihood'][i]:.4f}, "
                  f"{'all' if res['is_greedy'][i] else 'not all'} of them the model's top-1")
        if "finish_reason" in res and tokenizer is not None:
            what = {"stop_token": f" (token {res['stop_match'][i]})", "stop_sequence": f" (stop sequence {res['stop_match'][i]})"}
            print(f"    finish reason: {res['finish_reason'][i]}{what.get(res['finish_reason'][i], '')}")
    tps = res["useful_tokens_per_sec"]
    print(f"{len(reqs)} requests, {res['useful_tokens']} useful tokens in {res['wall_s']:.2f} s: {tps:.2f} tokens/sec; "
          f"{res['steps']} steps, {res['mean_active_slots']:.2f} active slots of {B} on average, "
          f"{100 * res['admission_share']:.1f} % of the time in {res['admissions']} admissions")
    if "kept_by_request" in res:
        for i, k in enumerate(res["kept_by_request"]):
            lv = args.sparsity if reqs[i].sparsity is None else reqs[i].sparsity
            print(f"    request {i}: sparsity {lv:g}, kept " + ("-" if k is None else f"{100 * k:.1f} %") + " of the rows on average")
    if prefixes:
        print(f"{res['prefix_admissions']} admissions on a shared prefix reused {res['prefix_rows_reused']} rows; suffix passes: "
              f"{res['prefix_paths']}")
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB")
    return {"tokens_per_sec": [tps], "mean_tokens_per_sec": tps, "useful_tokens_per_sec": tps, "batch_size": B, "thresholds": thresholds,
            "decoder": type(batcher).__name__, "sequences": res["tokens"], "steps": res["steps"], "admissions": res["admissions"],
            "admission_share": res["admission_share"], "mean_active_slots": res["mean_active_slots"], "union_kept": res["union_kept"],
            "sync_every": res["sync_every"], "prefix_admissions": res["prefix_admissions"],
            "prefix_rows_reused": res["prefix_rows_reused"], "prefix_paths": res["prefix_paths"], "kv_cache_bytes": kvb,
            **{k: res[k] for k in ("logprobs", "top_logprobs", "finish_reason", "stop_match", "kept_by_request", "forced", "loglikelihood",
                                    "is_greedy") if k in res}}


def sample_batch(logits: torch.Tensor, temperature: float, top_k: Optional[int]) -> torch.Tensor:
    """one token per row of logits [B, V] (generate.sample's rule, row by row)"""
    return torch.cat([sample(logits[b:b + 1].unsqueeze(0), temperature=temperature, top_k=top_k)[0].view(1) for b in range(logits.shape[0])])


def main(args) -> Dict:
    device = args.device
    assert "cuda" in device, "the sparse decode path is GPU-only (HIP kernels, no CPU fallback)"
    spec = check_speculative_args(args)  # before anything is loaded
    batch = check_batched_args(args)
    n_lp = check_logprobs_args(args)
    proc = check_processor_args(args)
    samp = check_sampling_args(args)
    check_stop_args(args)
    check_kv_cache_args(args)
    if getattr(args, "prefixes", None) is not None and getattr(args, "requests", None) is None:
        raise SystemExit("--prefixes names shared prefixes of continuous batching: it needs --requests")
    if getattr(args, "constraints", None) is not None and getattr(args, "requests", None) is None:
        raise SystemExit("--constraints names token automata of continuous batching: it needs --requests (an automaton starts at an "
                         "admission and ends on the request's EOS id)")
    if getattr(args, "requests", None) is not None:
        check_requests_args(args)
        request_lines, prefix_lines, constraints, levels = check_request_files(args)
    if getattr(args, "interactive", False) and args.synthetic:
        raise SystemExit("--interactive needs a tokenizer (a checkpoint directory), not --synthetic")
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.precision]
    # tensor parallelism as in the reference (gpt-fast/generate.py:249-256, tp.py): one process per GPU under
    # torch.distributed.run; FIRST, so that every rank builds / loads its shard on its own device.  A single process (the
    # north-star configuration) is untouched
    from teal_amd.gpt_fast import tp
    tp_rank = tp.maybe_init_dist()
    shard = None
    if tp_rank is not None:
        device = f"cuda:{torch.cuda.current_device()}"
        shard = tp.apply_tp  # wqkv / w1 / w3 column-wise, wo / w2 row-wise, one all-reduce per attention and per MLP
        if tp_rank != 0:
            import builtins
            builtins.print = lambda *a, **k: None  # rank 0 reports (tp.py's `print` override)
    from teal_amd import runtime
    runtime.init()
    t0 = time.time()
    if args.synthetic:
        model = build_synthetic_model(args.synthetic, device, dtype, n_layer=args.n_layer, shard=shard)
        prompt = torch.randint(0, model.config.vocab_size, (6,), device=device, dtype=torch.int,
                               generator=torch.Generator(device=device).manual_seed(7))  # "Hello, my name is" + BOS = 6 ids
        tokenizer = None
    else:
        assert args.checkpoint_path.is_file(), args.checkpoint_path
        model = load_checkpoint_model(args.checkpoint_path, device, dtype, shard=shard)
        from teal_amd.gpt_fast.tokenizer import get_tokenizer
        tokenizer = get_tokenizer(args.checkpoint_path.parent / "tokenizer.model", args.checkpoint_path)
        prompt = torch.tensor([tokenizer.bos_id()] + tokenizer.encode(args.prompt), dtype=torch.int, device=device)
    thresholds = None
    level_ths = None
    if getattr(args, "requests", None) is not None and any(lv != float(args.sparsity) for lv in levels):
        print(f"Resolving the requests' sparsity levels {levels} ...")
        level_ths = resolve_sparsity_levels(args, model, [lv for lv in levels if lv != float(args.sparsity)])
    if not args.dense and (args.hist_path is not None or args.synthetic):
        # like the reference, patching is gated on hist_path, not on sparsity (generate.py:328)
        print("Monkeypatching with activation sparsity...")
        thresholds = apply_sparsity(model, sparsity=args.sparsity, hist_path=args.hist_path,
                                    greedy_lookup=args.greedy_lookup, synthetic=bool(args.synthetic))
    if getattr(args, "no_fused_decode", False):
        model.fused_decode = False
    torch.cuda.synchronize()
    print(f"Time to load model: {time.time() - t0:.02f} seconds")
    torch.manual_seed(1234)
    if spec is not None:
        return run_speculative(args, model, thresholds, prompt, tokenizer, spec, device, dtype)
    if getattr(args, "requests", None) is not None:
        if level_ths is not None and 0.0 in level_ths:
            from teal_amd.gpt_fast.score import dense_thresholds
            level_ths[0.0] = dense_thresholds(thresholds)
        return run_continuous(args, model, thresholds, tokenizer, request_lines, prefix_lines, constraints, level_ths)
    if batch > 1:
        if args.synthetic:  # B distinct seeded prompts of equal length
            prompts = torch.randint(0, model.config.vocab_size, (batch, prompt.numel()), device=device, dtype=torch.int,
                                    generator=torch.Generator(device=device).manual_seed(7))
            prompts[0] = prompt
        else:  # the prompt repeated B times (gpt-fast's batched generate)
            prompts = prompt.view(1, -1).repeat(batch, 1)
        use_engine = thresholds is not None and (args.engine or (args.compile and not getattr(args, "no_engine", False)))
        return run_batched(args, model, thresholds, prompts, tokenizer, use_engine)
    model_size = _get_model_size(model)
    # a hipGraph holds the step only if the ranks' all-reduce can be captured (RCCL); a host-staged gloo reduce decodes eagerly
    # (TEAL_TP_GRAPH=0 keeps a sharded model's decode eager even over RCCL; a capture that fails falls back by itself)
    use_graph = args.compile and (tp_rank is None or (bool(getattr(getattr(model, "tp_reduce", None), "capturable", False))
                                                      and os.environ.get("TEAL_TP_GRAPH", "1") != "0"))
    decoder = GraphedDecoder(model, use_graph, args.temperature, args.top_k)
    use_engine = args.engine or (args.compile and thresholds is not None and not getattr(args, "no_engine", False))
    if use_engine and not args.engine:
        # --compile implies the device-resident engine loop only for models the fused step can run (int4 blocks, head_dim 48,
        # ... decode through the patched modules under the same hipGraph capture instead)
        from teal_amd.gpt_fast.engine import pick_engine
        _, why = pick_engine(model, need_caches=False)
        if why is not None:
            print(f"fused engine not used: {why}")
            use_engine = False
    if use_engine:
        assert thresholds is not None, "--engine needs thresholds (--hist_path or --synthetic)"
        decoder = EngineDecoder(model, thresholds, use_graph, args.temperature, args.top_k)
        relayout_for_engine(model)
    if n_lp is not None and not use_engine:
        raise SystemExit("--logprobs: the fused engine cannot run this model, and the module path returns token ids only")
    if proc and not use_engine:
        raise SystemExit("logit processors: the fused engine cannot run this model, and the module path samples from the raw logits")
    if samp and not use_engine:
        raise SystemExit("--top_p / --min_p: the fused engine cannot run this model, and the module path's sampler knows temperature "
                         "and top_k only")
    # --compile captures the prompt pass as well (one hipGraph per prompt length; the reference compiles `prefill` only under
    # --compile_prefill, generate.py:423-425 — its Inductor compile takes minutes, a capture here takes milliseconds, and the
    # eager pass is ~400 launches = nine decode steps' worth for a 6-token prompt).  The prefill stays DENSE
    # (kernels/sparse_gemv.py:271,298).  --eager_prefill keeps the op-by-op pass; a host-staged TP all-reduce cannot be captured.
    want_graph_prefill = (getattr(args, "compile_prefill", False) or args.compile) and not getattr(args, "eager_prefill", False)
    prefill = GraphedPrefill(model) if (want_graph_prefill and use_graph) else None
    if thresholds is not None and want_graph_prefill and not getattr(args, "module_prefill", False):
        # prompts of up to 8 tokens: the hand-fused HIP prompt pass (teal_amd/gpt_fast/prefill.py: eight launches per layer over
        # the decode step's weight images, dense); longer prompts, quantised or sharded models: the pass above
        from teal_amd.gpt_fast.prefill import FusedPrefill
        prefill = FusedPrefill(model, graph=use_graph, fallback=prefill)
    tps, seqs, lps, tops, lp_offsets = [], [], [], [], []
    start = -1 if args.compile else 0
    for i in range(start, args.num_samples):
        if getattr(args, "interactive", False) and i >= 0:
            text = input("What is your prompt? ")
            if "chat" in str(args.checkpoint_path):
                text = f"[INST] {text.strip()} [/INST]"
            prompt = torch.tensor([tokenizer.bos_id()] + tokenizer.encode(text), dtype=torch.int, device=device)
        torch.cuda.synchronize()
        prof = contextlib.nullcontext()
        if args.profile and i == args.num_samples - 1:
            prof = torch.profiler.profile()
        t0 = time.perf_counter()
        with prof:
            if n_lp is not None:
                # (the engine is built on the caches generate() is about to set up — the same sizes — and rebuilt when they move)
                model.setup_caches(max_batch_size=1, max_seq_length=min(prompt.size(0) + args.max_new_tokens, model.config.block_size))
                if decoder.model._lp is None:
                    decoder.model.set_logprobs(n_lp)
            y = generate(model, prompt, args.max_new_tokens, decoder, temperature=args.temperature, top_k=args.top_k,
                         prefill=prefill, processors=proc or None, sampling=samp or None)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if i == -1:
            print(f"Graph capture + warm-up time: {t:.2f} seconds")
            continue
        if hasattr(prof, "export_chrome_trace"):
            prof.export_chrome_trace(f"{args.profile}.json")
        n_gen = y.size(0) - prompt.size(0)
        tps.append(n_gen / t)
        seqs.append(y.tolist())
        if tokenizer is not None:
            print(tokenizer.decode(y.tolist()))
        if n_lp is not None:  # of the tokens the fused sampler drew: the last `drawn` of y (all the new ones on the usual path)
            eng = decoder.model
            drawn = int(eng.rng_state[1].item())
            lp, ids, tlp = eng.read_logprobs(0, drawn)
            lps.append(lp.tolist())
            tops.append([list(zip(a, b_)) for a, b_ in zip(ids.tolist(), tlp.tolist())])
            lp_offsets.append(y.size(0) - drawn)
            if tokenizer is not None:
                print(_mean_logprob_line(lps[-1]))
        print(f"Time for inference {i + 1}: {t:.02f} sec total, {tps[-1]:.02f} tokens/sec")
        print(f"Bandwidth achieved: {model_size * tps[-1] / 1e9:.02f} GB/s (dense parameter bytes x tok/s, as the reference reports)")
    print("==========")
    if thresholds is not None and args.report_kept:
        report_kept_fractions(model, thresholds, prompt)
        if use_engine and args.max_new_tokens > 4:
            eng = decoder.model  # all seven projections, on the DECODE activations of the generated range
            kf = eng.mean_kept_fractions(prompt[-1:].clone(), prompt.numel(), min(args.max_new_tokens - 1, eng.max_seq - prompt.numel()), 3)
            print("achieved kept fraction (decode activations):", {k: round(v, 3) for k, v in kf.items()})
    mean = sum(tps) / max(1, len(tps))
    print(f"Average tokens/sec: {mean:.2f}")
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB")
    pre_name = None if prefill is None else type(prefill).__name__ + (f":{prefill.used}" if getattr(prefill, "used", None) else "")
    return {"tokens_per_sec": tps, "mean_tokens_per_sec": mean, "thresholds": thresholds, "decoder": type(decoder).__name__,
            "sequences": seqs, "prefill": pre_name,
            **({"logprobs": lps, "logprob_offset": lp_offsets} if n_lp is not None else {}), **({"top_logprobs": tops} if n_lp else {})}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="TEAL decode harness (MI355X / HIP)")
    p.add_argument("--prompt", type=str, default="Hello, my name is")
    p.add_argument("--interactive", action="store_true", help="ask for a prompt before every sample (needs a tokenizer: not with "
                   "--synthetic); chat checkpoints get the reference's [INST] wrapping (generate.py:440-446)")
    p.add_argument("--num_samples", type=int, default=5)
    p.add_argument("--max_new_tokens", type=int, default=200)
    p.add_argument("--top_k", type=int, default=200)
    p.add_argument("--temperature", type=float, default=0.8)
    p.add_argument("--checkpoint_path", type=Path, default=Path("checkpoints/meta-llama/Llama-2-7b-chat-hf/model.pth"))
    p.add_argument("--compile", action="store_true", help="capture the decode step into a hipGraph")
    p.add_argument("--compile_prefill", action="store_true", help="capture the prompt pass into a hipGraph too "
                   "(the reference's flag of the same name, generate.py:540); implied by --compile here")
    p.add_argument("--eager_prefill", action="store_true", help="with --compile: keep the prompt pass op by op (no prefill graph)")
    p.add_argument("--module_prefill", action="store_true", help="with --compile: the prompt pass through the patched modules (under a "
                   "hipGraph) also for prompts of up to 8 tokens, instead of the hand-fused HIP prompt pass")
    p.add_argument("--profile", type=Path, default=None)
    p.add_argument("--speculate_k", type=int, default=5, help="speculative decoding: draft tokens per round (1..15)")
    p.add_argument("--draft_checkpoint_path", type=Path, default=None, help="speculative decoding: the TEAL-sparse draft model (the "
                   "target verifies dense); the target's own checkpoint path selects self-speculation")
    p.add_argument("--self_speculate", action="store_true", help="speculative decoding with the target's own weights as the TEAL-sparse "
                   "draft (--synthetic runs, which have no checkpoint path)")
    p.add_argument("--device", type=str, default=default_device)
    # monkeypatch (reference flags)
    p.add_argument("--hist_path", type=str, default=None)
    p.add_argument("--sparsity", type=float, default=0.0)
    # extensions
    p.add_argument("--precision", choices=["fp16", "bf16"], default="fp16")
    p.add_argument("--greedy_lookup", type=str, default=None, help="models/<name>/lookup directory (block-wise greedy sparsities)")
    p.add_argument("--synthetic", type=str, default=None, help="architecture name, e.g. 7B, llama-3-8b, 70B")
    p.add_argument("--n_layer", type=int, default=None, help="override the layer count (synthetic smoke runs)")
    p.add_argument("--dense", action="store_true", help="do not monkeypatch: dense baseline")
    p.add_argument("--report_kept", action="store_true", help="print the achieved kept fraction per projection")
    p.add_argument("--engine", action="store_true", help="fused HIP decode step (teal_amd/gpt_fast/engine.py); implied by --compile "
                   "when thresholds are installed")
    p.add_argument("--no_engine", action="store_true", help="with --compile: drive the patched model exactly as the reference "
                   "harness does (model(token, pos) -> torch sampler, captured in a hipGraph) instead of the device-resident "
                   "engine loop; single-token calls still run the fused HIP decode step (Transformer.fused_decode)")
    p.add_argument("--batch_size", type=int, default=1, help="batched decode: B <= 8 sequences per step (the prompt repeated B "
                   "times; --synthetic: B seeded prompts); through BatchedDecodeEngine under --compile / --engine")
    p.add_argument("--no_fused_decode", action="store_true", help="op-by-op module path (torch.ops.teal.* + eager glue) for "
                   "single-token calls: A/B against the fused decode step")
    p.add_argument("--requests", type=Path, default=None, help="continuous batching: a JSON Lines file, one request per line "
                   "({\"tokens\": [...]} or {\"prompt\": \"...\"}, optional \"max_new_tokens\"); --batch_size slots, refilled as "
                   "requests finish.  A line may carry \"forced_tokens\": [ids] (or \"forced_text\"): its first draws yield these "
                   "tokens and their log-likelihood is reported")
    p.add_argument("--prefixes", type=Path, default=None, help="with --requests: a JSON Lines file of shared prefixes, one per line "
                   "({\"id\": \"sys\", \"tokens\": [...]} or {\"id\": \"sys\", \"prompt\": \"...\"}); a request line that carries "
                   "\"prefix\": \"sys\" gives only its own suffix and reuses the prefix's K / V rows, computed once")
    p.add_argument("--constraints", type=Path, default=None, help="with --requests: a JSON Lines file of token automata, one per line "
                   "({\"id\": \"yes-no\", \"states\": [{\"edges\": [[token, next], ...], \"default\": -1, \"accept\": true}, ...]}, state 0 "
                   "the start); a request line that carries \"constraint\": \"yes-no\" draws every token under it.  Request lines "
                   "may also carry \"choices\" or \"allowed_token_ids\" without this file")
    p.add_argument("--eos_id", type=int, default=None, help="with --requests: a request also ends right after this token id (off "
                   "by default: budgets alone end requests)")
    p.add_argument("--logprobs", type=int, default=None, help="return each generated token's log-probability under the model's own "
                   "distribution (temperature 1, no top-k filter) and the N most likely alternates (0..8; 0: the token's only); "
                   "engine paths only: --compile / --engine, --batch_size, --requests")
    p.add_argument("--repetition_penalty", type=float, default=None, help="logit processor (engine paths only, like --logprobs): the "
                   "logit of every token of the prompt or generated so far is divided by this if positive, multiplied otherwise "
                   "(> 0; 1: off).  With --requests: the default of requests that set none")
    p.add_argument("--presence_penalty", type=float, default=None, help="logit processor: subtracted once from the logit of every "
                   "token generated so far (0: off)")
    p.add_argument("--frequency_penalty", type=float, default=None, help="logit processor: subtracted from a token's logit once per "
                   "time it was generated so far (0: off)")
    p.add_argument("--top_p", type=float, default=None, help="nucleus sampling (engine paths only, like --logprobs): after temperature "
                   "and top_k, keep the most likely tokens until their share of the kept mass reaches this (> 0; 1: off).  With "
                   "--requests: the default of requests that set none")
    p.add_argument("--min_p", type=float, default=None, help="min-p sampling: after top_p, keep the tokens at least this likely "
                   "relative to the most likely one (in [0, 1); 0: off)")
    p.add_argument("--kv_cache", type=str, default="model", choices=("model", "fp8"), help="with --requests: the slots' KV cache. "
                   "model: the model's 16-bit dtype.  fp8: e4m3 rows with one power-of-two scale per row and KV head, about half the "
                   "bytes per slot and per step; the prompt pass and a row's own step see exact K / V, later steps see fp8")
    p.add_argument("--stop_token_ids", type=str, default=None, help="with --requests: token ids a,b,c (at most 16) — a request also "
                   "ends right after any of them, like --eos_id.  The default of requests that set no \"stop_token_ids\"; a request "
                   "line may also carry \"stop_sequences\" (token id lists) and, with a tokenizer, \"stop\" strings (matched as the "
                   "token ids the tokenizer gives them: another spelling of the same text is not caught)")
    p.add_argument("--min_new_tokens", type=int, default=None, help="with --requests: no stop id, EOS id or stop sequence ends a request "
                   "before it produced this many tokens (its budget still does).  The default of requests that set none")
    p.add_argument("--finish_reason", action="store_true", help="with --requests: report why each request ended (stop_token / "
                   "stop_sequence / length / cache) even when no request carries a stop condition")
    p.add_argument("--sync_every", type=int, default=8, help="with --requests: steps per burst between two looks at the slot state")
    return p


if __name__ == "__main__":
    res = main(build_parser().parse_args())
    print(json.dumps({"mean_tokens_per_sec": res["mean_tokens_per_sec"]}))
