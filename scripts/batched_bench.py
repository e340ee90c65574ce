"""Batched decode on a synthetic model: ms per step and aggregate tok/s at B = 1, 2, 4, 8, the union's kept fraction per
projection, weight bytes per step / step time, the same engine with every row kept, and DecodeEngine at B = 1 — one process.

    python scripts/batched_bench.py --synthetic 7B --precision fp16 --sparsity 0.5
    python scripts/batched_bench.py --synthetic llama-3-8b --precision bf16 --sparsity 0.4

A step is one hipGraph replay (the forward pass of all B sequences and B sampler launches), timed over --steps replays.  Random
weights and activations: the union of B sequences' kept rows grows like 1 - (1 - keep)^B; a real checkpoint's shared outlier
channels should keep fewer, which random weights cannot show.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from teal_amd import runtime  # noqa: E402
from teal_amd.gpt_fast import generate as G  # noqa: E402
from teal_amd.gpt_fast.batched import BatchedDecodeEngine  # noqa: E402
from teal_amd.gpt_fast.engine import DecodeEngine  # noqa: E402


def replay_ms(g, steps):
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--synthetic", default="7B")
    p.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--sparsity", type=float, default=0.5)
    p.add_argument("--batches", default="1,2,4,8")
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--pos", type=int, default=32, help="position of the first timed step")
    a = p.parse_args()
    runtime.init()
    dev, dt = "cuda", {"fp16": torch.float16, "bf16": torch.bfloat16}[a.precision]
    m = G.build_synthetic_model(a.synthetic, dev, dt)
    ths = G.apply_sparsity(m, sparsity=a.sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
    dense = [{k: float("-inf") for k in t} for t in ths]
    max_seq = a.pos + 2 * a.steps + 8
    V = m.config.vocab_size
    g = torch.Generator(device=dev).manual_seed(0)
    head = {"model": a.synthetic, "precision": a.precision, "sparsity": a.sparsity, "steps": a.steps, "pos": a.pos}
    print(json.dumps(head))
    # the single-sequence engine first (its caches are [1, ...])
    m.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    e1 = DecodeEngine(m, ths)
    e1.tok_buf.copy_(torch.randint(0, V, (1, 1), device=dev, generator=g))
    e1.pos_buf.fill_(a.pos)
    ms1 = replay_ms(e1.capture_loop(0.8, 200), a.steps)
    print(json.dumps({"leg": "DecodeEngine", "B": 1, "ms_per_step": round(ms1, 3), "tok_s": round(1e3 / ms1, 1)}))
    del e1
    for B in [int(x) for x in a.batches.split(",")]:
        m.max_seq_length, m.max_batch_size = -1, -1
        m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
        for name, t in (("batched", ths), ("batched_dense", dense)):
            eng = BatchedDecodeEngine(m, t, B)
            eng.tok_buf[:B].copy_(torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32))
            eng.pos_buf[:B].copy_(torch.arange(a.pos, a.pos + B, device=dev, dtype=torch.int32))
            ms = replay_ms(eng.capture(0.8, 200), a.steps)
            eng._step()  # one more eager step for the counts (the graph's buffers are the same)
            torch.cuda.synchronize()
            kf = eng.kept_fractions()
            nbytes = eng.weight_bytes_per_step()
            rec = {"leg": name, "B": B, "ms_per_step": round(ms, 3), "tok_s": round(B * 1e3 / ms, 1),
                   "x_vs_DecodeEngine": round(B * ms1 / ms, 2), "weight_GB_per_step": round(nbytes / 1e9, 3),
                   "weight_TB_s": round(nbytes / ms / 1e9, 2),
                   "union_kept": {k: round(v["union"], 3) for k, v in kf.items()},
                   "per_seq_kept": {k: round(v["per_seq"], 3) for k, v in kf.items()}}
            print(json.dumps(rec))
            del eng
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
