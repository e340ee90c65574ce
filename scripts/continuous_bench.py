"""Continuous batching on a synthetic model: useful tok/s of ContinuousBatcher against static batching (refill="all") on the same
engine at B = 4 and 8, alternated in one process, and against sequential single-stream DecodeEngine runs of the same requests.

    python scripts/continuous_bench.py --synthetic 7B --precision fp16 --sparsity 0.5
    python scripts/continuous_bench.py --synthetic llama-3-8b --precision bf16 --sparsity 0.4

Workload: --n requests from a fixed seed, prompt lengths uniform in --prompt (4..16: the HIP prompt pass; 17..128: the module
path) and budgets uniform in 16..256.  Useful tokens are those inside a request's budget.  Per leg: useful tok/s, wall time, steps,
mean active slots, the share of device time spent in admissions, and the union kept fraction per projection (the last step of
every burst, active slots only).

--shared_prefix P instead: every request names ONE P-token prefix, with suffixes uniform in 4..16 tokens and the same budgets.  Two
legs on the same engine, alternated: "shared" (the prefix registered: an admission is one row copy and a HIP pass over the suffix)
and "unshared" (the same requests with prefix + suffix as plain tokens: the module path).  Per leg also ms per admission.

    python scripts/continuous_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --shared_prefix 100
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
from teal_amd.gpt_fast.batched import SlotDecodeEngine  # noqa: E402
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request  # noqa: E402


def workload(n, prompt, budget, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = prompt
    out = []
    for _ in range(n):
        T = int(torch.randint(lo, hi + 1, (1,), generator=g))
        out.append(Request(torch.randint(0, vocab, (T,), generator=g).tolist(), int(torch.randint(budget[0], budget[1] + 1, (1,), generator=g))))
    return out


def rec(leg, B, variant, res):
    return {"leg": leg, "B": B, "prompts": variant, "useful_tok_s": round(res["useful_tokens_per_sec"], 1), "wall_s": round(res["wall_s"], 2),
            "steps": res["steps"], "mean_active_slots": round(res["mean_active_slots"], 2),
            "admission_share": round(res["admission_share"], 3), "union_kept": {k: round(v, 3) for k, v in res["union_kept"].items()}}


def shared_prefix(a, m, ths, V):
    """--shared_prefix: the same 64 requests with the prefix's rows reused ("shared") and recomputed per request ("unshared")"""
    P = a.shared_prefix
    prefix = torch.randint(0, V, (P,), generator=torch.Generator().manual_seed(5)).tolist()
    sfx = workload(a.n, (4, 16), (16, 256), V, 7)
    shared = [Request(r.tokens, r.max_new_tokens, prefix="sys") for r in sfx]
    unshared = [Request(prefix + r.tokens, r.max_new_tokens) for r in sfx]
    max_seq = max(len(r.tokens) + r.max_new_tokens for r in unshared)
    name = f"{P}+4..16"
    print(json.dumps({"prompts": name, "useful_tokens": sum(r.max_new_tokens for r in sfx), "max_seq": max_seq}), flush=True)
    for B in [int(x) for x in a.batches.split(",")]:
        m.max_seq_length, m.max_batch_size = -1, -1
        m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
        eng = SlotDecodeEngine(m, ths, B)
        with_pf = ContinuousBatcher(eng, sync_every=a.sync_every, refill="free", prefixes={"sys": prefix})
        without = ContinuousBatcher(eng, sync_every=a.sync_every, refill="free")
        with_pf.run(shared[:B + 2])  # warm-up: registration, graph capture, both admission paths
        without.run(unshared[:B + 2])
        for leg, bt, reqs in (("shared", with_pf, shared), ("unshared", without, unshared)) * 2:
            eng.reset_stats()
            res = bt.run(reqs)
            assert [len(t) for t in res["tokens"]] == [r.max_new_tokens for r in reqs]
            r = rec(leg, B, name, res)
            r["ms_per_admission"] = round(1e3 * res["admission_s"] / res["admissions"], 3)
            r["admit_paths"], r["prefix_paths"], r["prefix_MB"] = dict(eng.admit_paths), dict(eng.prefix_paths), round(eng.prefix_bytes() / 1e6, 1)
            print(json.dumps(r), flush=True)
        del eng, with_pf, without
        torch.cuda.empty_cache()


def sequential(m, ths, reqs, max_seq, temperature, top_k):
    """each request alone: the HIP prompt pass (or the module path) and DecodeEngine's device-resident loop, as generate.py runs"""
    from teal_amd.gpt_fast.prefill import FusedPrefill
    m.max_seq_length, m.max_batch_size = -1, -1
    m.setup_caches(max_batch_size=1, max_seq_length=max_seq)
    dec = G.EngineDecoder(m, ths, True, temperature, top_k)
    G.relayout_for_engine(m)
    pre = FusedPrefill(m, graph=True)
    dev = m.output.weight.device
    G.generate(m, torch.tensor(reqs[0].tokens, dtype=torch.int, device=dev), 4, dec, temperature, top_k, prefill=pre)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for r in reqs:
        y = G.generate(m, torch.tensor(r.tokens, dtype=torch.int, device=dev), r.max_new_tokens, dec, temperature, top_k, prefill=pre)
        n += y.numel() - len(r.tokens)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    return {"leg": "DecodeEngine_sequential", "B": 1, "useful_tok_s": round(n / t, 1), "wall_s": round(t, 2), "useful_tokens": n}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--synthetic", default="7B")
    p.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--sparsity", type=float, default=0.5)
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--batches", default="4,8")
    p.add_argument("--variants", default="4-16,17-128")
    p.add_argument("--sync_every", type=int, default=8)
    p.add_argument("--sequential", action="store_true", help="also the sequential DecodeEngine leg (first variant)")
    p.add_argument("--shared_prefix", type=int, default=0, help="P > 0: the shared-prefix comparison instead (every request on one "
                   "P-token prefix, suffixes 4..16)")
    a = p.parse_args()
    runtime.init()
    dev, dt = "cuda", {"fp16": torch.float16, "bf16": torch.bfloat16}[a.precision]
    m = G.build_synthetic_model(a.synthetic, dev, dt)
    ths = G.apply_sparsity(m, sparsity=a.sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
    V = m.config.vocab_size
    print(json.dumps({"model": a.synthetic, "precision": a.precision, "sparsity": a.sparsity, "requests": a.n, "budgets": "16..256",
                      "sync_every": a.sync_every}), flush=True)
    if a.shared_prefix > 0:
        return shared_prefix(a, m, ths, V)
    variants = [tuple(int(x) for x in v.split("-")) for v in a.variants.split(",")]
    for vi, pr in enumerate(variants):
        reqs = workload(a.n, pr, (16, 256), V, 7 + vi)
        max_seq = max(len(r.tokens) + r.max_new_tokens for r in reqs)
        name = f"{pr[0]}..{pr[1]}"
        print(json.dumps({"prompts": name, "useful_tokens": sum(r.max_new_tokens for r in reqs), "max_seq": max_seq}), flush=True)
        for B in [int(x) for x in a.batches.split(",")]:
            m.max_seq_length, m.max_batch_size = -1, -1
            m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
            eng = SlotDecodeEngine(m, ths, B)
            cont = ContinuousBatcher(eng, sync_every=a.sync_every, refill="free")
            stat = ContinuousBatcher(eng, sync_every=a.sync_every, refill="all")
            cont.run(reqs[:B + 2])  # warm-up: graph capture, both admission paths
            for leg, bt in (("continuous", cont), ("refill_all", stat), ("continuous", cont), ("refill_all", stat)):
                eng.reset_stats()
                res = bt.run(reqs)
                assert [len(t) for t in res["tokens"]] == [r.max_new_tokens for r in reqs]
                r = rec(leg, B, name, res)
                r["admit_paths"] = dict(eng.admit_paths)
                print(json.dumps(r), flush=True)
            del eng, cont, stat
            torch.cuda.empty_cache()
        if a.sequential and vi == 0:
            r = sequential(m, ths, reqs, max_seq, 0.8, 200)
            r["prompts"] = name
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
