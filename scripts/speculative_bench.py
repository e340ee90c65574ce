"""Speculative decoding on a synthetic model: the round's cost split and tokens/sec with the acceptance histogram.

    python scripts/speculative_bench.py --synthetic 7B --precision fp16 --k 4 --sparsity 0.5 --max_new_tokens 200

Legs, all in one process on the same random weights (acceptance on random weights says nothing about a real checkpoint's):
  * dense engine   DecodeEngine at sparsity 0, one hipGraph replay per token
  * sparse engine  DecodeEngine at --sparsity
  * self-spec      SpeculativeDecoder, draft = the model at --sparsity, dense verify; and at draft sparsity 0 (accepts ~all: the
                   upper bound of what a round yields)
  * cost split     one round's launches timed separately with events: k draft steps / verify pass / accept
tok/s counts the new tokens over the whole generate call (prompt pass included), as the reference does.
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
from teal_amd.gpt_fast.engine import DecodeEngine  # noqa: E402
from teal_amd.gpt_fast.prefill import FusedPrefill  # noqa: E402
from teal_amd.gpt_fast.speculative import SpeculativeDecoder, VerifyPass  # noqa: E402


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def event_ms(fn, reps=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--synthetic", default="7B")
    p.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--k", type=int, default=4)
    p.add_argument("--sparsity", type=float, default=0.5)
    p.add_argument("--max_new_tokens", type=int, default=200)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--top_k", type=int, default=200)
    p.add_argument("--temperature", type=float, default=0.8)
    a = p.parse_args()
    runtime.init()
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[a.precision]
    m = G.build_synthetic_model(a.synthetic, "cuda", dt)
    th = G.apply_sparsity(m, sparsity=a.sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
    ths = {a.sparsity: th, 0.0: [{p: 0.0 for p in t} for t in th]}  # tau = 0: every nonzero activation kept (dense draft)
    prompt = torch.randint(0, m.config.vocab_size, (6,), device="cuda", dtype=torch.int, generator=torch.Generator(device="cuda").manual_seed(7))
    T, n = prompt.numel(), a.max_new_tokens
    m.setup_caches(max_batch_size=1, max_seq_length=T + n + a.k + 1)
    G.relayout_for_engine(m)
    pre = FusedPrefill(m, graph=True)
    verify = VerifyPass(m)
    res = {"model": a.synthetic, "precision": a.precision, "k": a.k, "max_new_tokens": n, "top_k": a.top_k, "temperature": a.temperature,
           "note": "synthetic random weights: acceptance rates say nothing about a real checkpoint's"}

    for s in sorted(ths):  # plain engine loops
        eng = DecodeEngine(m, ths[s])

        def plain():
            logits = pre(prompt)
            first = eng.sample_first(logits[0, -1].contiguous(), a.temperature, a.top_k)
            return eng.decode_n(first, T, n - 1, a.temperature, a.top_k, use_graph=True, drawn=1)
        plain()
        t, _ = timed(plain, a.reps)
        res[f"engine_sparsity_{s}_tok_s"] = round(n / t, 1)

    for s in sorted(ths):  # self-speculation with the draft at sparsity s
        eng = DecodeEngine(m, ths[s])
        spec = SpeculativeDecoder(eng, verify, a.k, a.temperature, a.top_k, fill_in=False, capacity=n + a.k + 1, graph=True)
        G.speculative_generate(spec, prompt, n, pre, None, a.temperature, a.top_k)
        hist = [0] * (a.k + 1)

        def run():
            seq, h = G.speculative_generate(spec, prompt, n, pre, None, a.temperature, a.top_k)
            for i, v in enumerate(h):
                hist[i] += v
            return seq
        t, _ = timed(run, a.reps)
        st = SpeculativeDecoder.acceptance_stats(hist)
        res[f"self_spec_draft_sparsity_{s}"] = {"tok_s": round(n / t, 1), "acceptance_histogram": hist,
                                               "acceptance_probs": [round(x, 4) for x in st["acceptance_probs"]],
                                               "mean_accepted": round(st["mean_accepted"], 3)}
        if s == a.sparsity:  # the round's cost split, eagerly per part (launch overhead included) and the whole round from its graph
            spec.begin(torch.tensor([1], device="cuda"), T)
            L, V, k = spec.L, m.config.vocab_size, a.k

            def drafts():
                for j in range(k):
                    eng(spec.tokens[j:j + 1].view(1, 1), eng.pos_buf, logits_out=spec.dlog[j])
                    L.teal_sample_topk_ws(spec.dlog[j].data_ptr(), V, eng.code, a.top_k, a.temperature, eng.rng_state.data_ptr(),
                                          spec.tokens[j + 1:].data_ptr(), eng.pos_buf.data_ptr(), None, 0, eng.ws.data_ptr(),
                                          eng.ws.numel() * 4, runtime.stream_ptr())
                eng.pos_buf.copy_(spec.spec_pos)

            res["round_ms"] = {"k_draft_steps_eager": round(event_ms(drafts), 3),
                               "verify_pass_eager": round(event_ms(lambda: verify.run(spec.tokens, spec.spec_pos, k + 1)), 3)}
            ns = verify.run(spec.tokens, spec.spec_pos, k + 1)

            def accept():
                spec.spec_pos.fill_(T)
                spec.out_len.zero_()
                L.teal_spec_accept(verify.lm_slabs.data_ptr(), ns, spec.dlog.data_ptr(), V, k, eng.code, a.top_k, a.temperature,
                                   eng.rng_state.data_ptr(), spec.tokens.data_ptr(), spec.spec_pos.data_ptr(), None, spec.out_seq.data_ptr(),
                                   spec.capacity, spec.out_len.data_ptr(), spec.n_acc.data_ptr(), None, spec.scratch.data_ptr(),
                                   spec.scratch.numel() * 4, runtime.stream_ptr())
            res["round_ms"]["accept_eager_incl_two_fills"] = round(event_ms(accept), 3)
            g = spec.capture()

            def whole():
                spec.spec_pos.fill_(T)
                eng.pos_buf.fill_(T)
                spec.out_len.zero_()
                g.replay()
            res["round_ms"]["whole_round_graph_incl_three_fills"] = round(event_ms(whole), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
