"""Perplexity of the fused decode path under TEAL sparsity, on the caller's own token ids.

    python -m teal_amd.gpt_fast.score (--synthetic NAME | --checkpoint_path P)
        [--hist_path H --sparsity S | --greedy_lookup ...] --tokens FILE [--window W] [--batch_size B]

FILE is JSON Lines of {"tokens": [...]} (with a tokenizer — a checkpoint — {"text": "..."} too).  Each sequence is cut into
windows of at most W tokens (default: the cache length, the model's block_size) and each window is scored by teacher forcing
from an empty cache (DecodeEngine.score: one hipGraph replay per position).  Two numbers are printed, token-weighted perplexity
exp(-sum lp / n) over the same windows on the same engine:

  * at the given sparsity, and
  * with every threshold at -1 (every row kept): the dense model on the same kernels.

What this number is.  EVERY position of a window — the context included — runs the decode step: our kernels, our threshold
compare, our 16-bit hand-overs, with the activations masked at the engine's thresholds.  The reference measures perplexity with
its HF path (teal/ppl_test.py: dense matmuls on masked activations) and, when it generates, runs the prompt pass dense and only
the decode steps sparse; here the context's K / V rows come from sparsified steps as well, so the ratio of the two numbers is
an upper bound on the damage sparsity does to generation after a dense prompt pass.  The logprobs are the model's own
distribution (temperature 1, no top-k filter).  A window's first token is conditioned on nothing and is not scored (a window of
T tokens gives T - 1 logprobs), so windows are not comparable with a sliding-context evaluation; a trailing window of one token
scores nothing.

--batch_size B (2..8) scores the same windows through continuous batching instead: each window w becomes a request with the prompt
[w[0]], forced_tokens w[1:] and no EOS id, B of them share the batched step (SlotDecodeEngine, ContinuousBatcher), and a window's
logprobs are those of its forced draws.  The two perplexities are printed as before, the second from a second engine at thresholds
-1.  What differs from the single-stream numbers: position 0 of a window goes through the admission's prompt pass (a one-token
prompt: the module path's op-by-op kernels, at the leg's thresholds) and not through the fused decode step, and the batched chain's
sums are grouped differently from the lean GEMV's (slabs summed in slice order, rounded once) — so the numbers are close to
DecodeEngine.score's, not identical.  Without the flag the tool is as it was.  No dataset ships with this repository and none is downloaded: the tool scores the token ids it is given.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence


def parse_sequences(lines: Sequence[str], tokenizer=None) -> List[List[int]]:
    """JSON Lines, one sequence per line: {"tokens": [...]} or {"text": "..."} (needs a tokenizer; BOS prepended as generate.py
    does for prompts).  Blank lines are skipped."""
    out = []
    for i, line in enumerate(lines):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
        except json.JSONDecodeError as e:
            raise ValueError(f"line {i + 1}: not JSON ({e})") from None
        if not isinstance(d, dict) or ("tokens" in d) == ("text" in d):
            raise ValueError(f"line {i + 1}: needs exactly one of \"tokens\" and \"text\"")
        if "tokens" in d:
            toks = d["tokens"]
            if not isinstance(toks, list) or not toks or not all(isinstance(t, int) and not isinstance(t, bool) and t >= 0 for t in toks):
                raise ValueError(f"line {i + 1}: \"tokens\" must be a non-empty list of token ids")
        else:
            if tokenizer is None:
                raise ValueError(f"line {i + 1}: a \"text\" needs a tokenizer (a checkpoint), not --synthetic")
            if not isinstance(d["text"], str):
                raise ValueError(f"line {i + 1}: \"text\" must be a string")
            toks = [tokenizer.bos_id()] + tokenizer.encode(d["text"])
        out.append([int(t) for t in toks])
    if not out:
        raise ValueError("no sequences")
    return out


def cut_windows(seqs: Sequence[Sequence[int]], window: int) -> List[List[int]]:
    """every sequence cut into consecutive windows of at most `window` tokens; windows of fewer than 2 tokens (nothing to
    score) are dropped"""
    if window < 2:
        raise ValueError(f"window must be at least 2 tokens, got {window}")
    out = []
    for s in seqs:
        for a in range(0, len(s), window):
            w = list(s[a:a + window])
            if len(w) >= 2:
                out.append(w)
    return out


def perplexity(logprobs: Sequence[Sequence[float]]) -> float:
    """token-weighted: exp(-sum lp / n) over every logprob of every window"""
    n = sum(len(w) for w in logprobs)
    if n == 0:
        raise ValueError("nothing was scored (every window is shorter than 2 tokens)")
    return math.exp(-math.fsum(v for w in logprobs for v in w) / n)


def score_windows(eng, windows: Sequence[Sequence[int]], use_graph: bool = True) -> List[List[float]]:
    import torch
    return [eng.score(torch.tensor(w, dtype=torch.int32), use_graph=use_graph).tolist() for w in windows]


def score_windows_batched(eng, windows: Sequence[Sequence[int]], use_graph: bool = True, sync_every: int = 8) -> List[List[float]]:
    """the windows as teacher-forced requests through ContinuousBatcher on a SlotDecodeEngine: window w is the prompt [w[0]] with
    forced_tokens w[1:] and no EOS id; -> per window the logprobs of its forced draws (len(w) - 1 of them)"""
    from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
    reqs = [Request([int(w[0])], len(w) - 1, None, forced_tokens=[int(t) for t in w[1:]]) for w in windows]
    res = ContinuousBatcher(eng, sync_every=sync_every, use_graph=use_graph, logprobs=1).run(reqs)
    short = [i for i, (k, w) in enumerate(zip(res["forced"], windows)) if k != len(w) - 1]
    if short:
        raise RuntimeError(f"window {short[0]} made {res['forced'][short[0]]} of its {len(windows[short[0]]) - 1} forced draws")
    return [lp[:len(w) - 1] for lp, w in zip(res["logprobs"], windows)]


def set_module_thresholds(model, ths: List[Dict[str, float]]) -> None:
    """the thresholds the patched modules' own forward (the admission pass of a one-token prompt) masks under"""
    for layer, th in zip(model.layers, ths):
        at, ff = layer.attention, layer.feed_forward
        at.thresh_q, at.thresh_k, at.thresh_v, at.thresh_o = (th[k] for k in ("q", "k", "v", "o"))
        ff.thresh_up, ff.thresh_gate, ff.thresh_down = th["up"], th["gate"], th["down"]


def dense_thresholds(ths: List[Dict[str, float]]) -> List[Dict[str, float]]:
    """every row kept: |x| > -1"""
    return [{p: -1.0 for p in th} for th in ths]


def main(args) -> Dict:
    import torch

    from teal_amd import runtime
    from teal_amd.gpt_fast import generate as G
    from teal_amd.gpt_fast.engine import pick_engine
    if (args.synthetic is None) == (args.checkpoint_path is None):
        raise SystemExit("score: give exactly one of --synthetic NAME and --checkpoint_path P")
    if args.synthetic is None and args.hist_path is None:
        raise SystemExit("score: a checkpoint needs --hist_path (the thresholds come from its activation histograms)")
    if not 0.0 <= args.sparsity < 1.0:
        raise SystemExit("score: --sparsity must be in [0, 1)")
    if args.window is not None and args.window < 2:
        raise SystemExit("score: --window must be at least 2 tokens")
    if args.batch_size is not None and not 2 <= args.batch_size <= 8:
        raise SystemExit("score: --batch_size must be in 2..8 (without it the windows are scored one at a time)")
    device = args.device
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.precision]
    runtime.init()
    if args.synthetic:
        model, tokenizer = G.build_synthetic_model(args.synthetic, device, dtype, n_layer=args.n_layer), None
    else:
        if not args.checkpoint_path.is_file():
            raise SystemExit(f"score: checkpoint {args.checkpoint_path} not found")
        model = G.load_checkpoint_model(args.checkpoint_path, device, dtype)
        from teal_amd.gpt_fast.tokenizer import get_tokenizer
        tokenizer = get_tokenizer(args.checkpoint_path.parent / "tokenizer.model", args.checkpoint_path)
    try:
        with open(args.tokens) as f:
            seqs = parse_sequences(f.read().splitlines(), tokenizer)
        bad = [t for s in seqs for t in s if t >= model.config.vocab_size]
        if bad:
            raise ValueError(f"token id {bad[0]} is outside the vocabulary of {model.config.vocab_size}")
        W = min(args.window or model.config.block_size, model.config.block_size)
        windows = cut_windows(seqs, W)
        if not windows:
            raise ValueError("every sequence is shorter than 2 tokens: nothing to score")
    except (OSError, ValueError) as e:
        raise SystemExit(f"--tokens: {e}")
    ths = G.apply_sparsity(model, sparsity=args.sparsity, hist_path=args.hist_path, greedy_lookup=args.greedy_lookup,
                           synthetic=bool(args.synthetic))
    model.max_seq_length, model.max_batch_size = -1, -1
    n = sum(len(w) - 1 for w in windows)
    if args.batch_size is not None:
        from teal_amd.gpt_fast.batched import SlotDecodeEngine
        B = int(args.batch_size)
        model.setup_caches(max_batch_size=B, max_seq_length=max(len(w) for w in windows))
        G.relayout_for_engine(model)
        why = SlotDecodeEngine.supports(model)
        if why is not None:
            raise SystemExit(f"score: --batch_size: the batched engine cannot run this model: {why}")
        sparse = perplexity(score_windows_batched(SlotDecodeEngine(model, ths, B), windows))
        set_module_thresholds(model, dense_thresholds(ths))
        dense = perplexity(score_windows_batched(SlotDecodeEngine(model, dense_thresholds(ths), B), windows))
        print(f"{len(windows)} windows of at most {W} tokens, {n} scored tokens (model distribution, temperature 1; {B} windows per "
              "batched step, position 0 of each through the prompt pass)")
        print(f"perplexity at sparsity {args.sparsity:g}: {sparse:.4f}")
        print(f"perplexity with every row kept (thresholds -1), same windows: {dense:.4f}")
        return {"perplexity": sparse, "perplexity_dense": dense, "windows": len(windows), "scored_tokens": n, "window": W, "batch_size": B}
    model.setup_caches(max_batch_size=1, max_seq_length=max(len(w) for w in windows))
    G.relayout_for_engine(model)
    cls, why = pick_engine(model)
    if cls is None:
        raise SystemExit(f"score: no fused engine for this model: {why}")
    eng = cls(model, ths)
    sparse = perplexity(score_windows(eng, windows))
    eng.set_thresholds(dense_thresholds(ths))
    dense = perplexity(score_windows(eng, windows))
    print(f"{len(windows)} windows of at most {W} tokens, {n} scored tokens (model distribution, temperature 1; every position "
          "through the sparse decode step)")
    print(f"perplexity at sparsity {args.sparsity:g}: {sparse:.4f}")
    print(f"perplexity with every row kept (thresholds -1), same engine and windows: {dense:.4f}")
    return {"perplexity": sparse, "perplexity_dense": dense, "windows": len(windows), "scored_tokens": n, "window": W}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="teacher-forced perplexity of the fused TEAL decode path on the caller's token ids")
    p.add_argument("--synthetic", type=str, default=None, help="architecture name (random weights), e.g. tiny-test, 7B")
    p.add_argument("--checkpoint_path", type=Path, default=None)
    p.add_argument("--n_layer", type=int, default=None, help="override the layer count (synthetic runs)")
    p.add_argument("--hist_path", type=str, default=None)
    p.add_argument("--sparsity", type=float, default=0.5)
    p.add_argument("--greedy_lookup", type=str, default=None, help="models/<name>/lookup directory (block-wise greedy sparsities)")
    p.add_argument("--tokens", type=Path, required=True, help="JSON Lines: {\"tokens\": [...]} or, with a tokenizer, {\"text\": \"...\"}")
    p.add_argument("--window", type=int, default=None, help="tokens per window (default: the model's block_size)")
    p.add_argument("--batch_size", type=int, default=None, help="2..8: score that many windows per batched step, as teacher-forced "
                   "requests of continuous batching (default: one window at a time on the single-stream engine)")
    p.add_argument("--precision", choices=["fp16", "bf16"], default="fp16")
    p.add_argument("--device", type=str, default="cuda")
    return p


if __name__ == "__main__":
    res = main(build_parser().parse_args())
    print(json.dumps(res))
    sys.exit(0)
