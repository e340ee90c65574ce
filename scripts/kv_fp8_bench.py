"""What the fp8 KV cache buys and costs: the continuous-batching step on the model's 16-bit caches (kv_cache=None, "model") against
SlotDecodeEngine(kv_cache="fp8"), on a synthetic model with the slots admitted at about --pos cached rows.

    python scripts/kv_fp8_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --pos 3800 --out profiles/kv_fp8_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  Both engines live side by side on one model (the 16-bit engine keeps
its caches; the model's own are then re-allocated at batch 1 as the fp8 engine's staging cache), the settings alternate, every
setting is run twice — the spread between a setting's two runs is the noise a difference has to beat — and every timed window
starts from the same tokens, positions, draw counters and slot state.

  leg 1  SlotDecodeEngine at B = 8, all slots active: ms per step, model | fp8, and the three byte figures of kv_cache_bytes()
  leg 2  SlotDecodeEngine with one slot: the same
  leg 3  the attention launch of layer 0 alone, at B = 8 and with one slot: a graph of --chain launches, ms per launch
  leg 4  admission at B = 8: ms per admit() of a prompt of about --pos tokens (the median of slots 1 .. 7; slot 0 warms the path up)
         on either engine — the fp8 engine's includes its teal_kv8_quantize_rows launch — and that launch alone over the same rows

--settings model --legs 1,2 runs on a library without the feature too (TEAL_LIB_PATH: the parent commit's build, for the model
setting's comparison in alternating processes).
"""
import statistics
import time

import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SlotDecodeEngine

T, TOP_K = 0.8, 200


def build(bench, m, ths, prompts, B, fmt):
    """an engine of B slots in format `fmt`, every slot admitted, its step graph and its attention-chain graph captured.  The
    model's caches of the moment are kept alive with it: the next engine re-allocates them."""
    bench.caches(m, B if fmt == "model" else 1)
    eng = SlotDecodeEngine(m, ths, B, **({} if fmt == "model" else {"kv_cache": fmt}))
    admit_ms = []
    for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.admit(s, prompts[s], bench.max_seq, None, 1234 + s, T, TOP_K)
        torch.cuda.synchronize()
        admit_ms.append((time.perf_counter() - t0) * 1e3)
    state = [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state]
    saved = [t.clone() for t in state]

    def reset():
        for t, v in zip(state, saved):
            t.copy_(v)

    g = eng.capture(T, TOP_K)
    reset()
    at, ns = m.layers[0].attention, eng.splits[0][0]
    chain = capture(lambda: [eng._attention(at, eng.slabs[0], ns, runtime.stream_ptr()) for _ in range(bench.a.chain)])
    return {"eng": eng, "step": g, "chain": chain, "reset": reset, "admit_ms": admit_ms, "B": B, "bytes": eng.kv_cache_bytes(),
            "caches": [layer.attention.kv_cache for layer in m.layers]}


def leg_pair(bench, m, ths, prompts, B, legs):
    name = f"SlotDecodeEngine B={B}"
    built = {fmt: build(bench, m, ths, prompts, B, fmt) for fmt in bench.settings}  # ("model" first: its graphs hold its own caches)
    if ("1" if B == 8 else "2") in legs:
        for rnd, fmt in bench.rounds():
            b = built[fmt]
            ms = replay_ms(b["step"], bench.a.steps, b["reset"])
            assert b["eng"].read_state()[SLOT_ACTIVE] == (1 << B) - 1, "a slot retired inside the timed window"
            bench.emit({"leg": name, "kv_cache": fmt, "run": rnd, "ms_per_step": round(ms, 4), "kv_cache_bytes": b["bytes"]})
    if "3" in legs:
        for rnd, fmt in bench.rounds():
            b = built[fmt]
            ms = replay_ms(b["chain"], max(10, bench.a.steps // 4), b["reset"]) / bench.a.chain
            bench.emit({"leg": f"attention launch alone, B={B}", "kv_cache": fmt, "run": rnd, "ms_per_launch": round(ms, 5)})
    if "4" in legs and B == 8:
        for fmt in bench.settings:
            a = built[fmt]["admit_ms"]
            bench.emit({"leg": "admission B=8", "kv_cache": fmt, "prompt_tokens": len(prompts[1]), "admit_ms_median_slots_1_7":
                        round(statistics.median(a[1:]), 3), "admit_ms_first": round(a[0], 3)})
        if "fp8" in built:
            eng, rows = built["fp8"]["eng"], len(prompts[7])  # (the staging cache holds slot 7's prompt: its rows go to slot 7 again)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                eng._quantize_rows(7, rows)
            e0.record()
            for _ in range(20):
                eng._quantize_rows(7, rows)
            e1.record()
            e1.synchronize()
            bench.emit({"leg": "teal_kv8_quantize_rows alone", "rows": rows, "ms_per_launch": round(e0.elapsed_time(e1) / 20, 5)})
    del built


def main():
    bench = FeatureBench("model,fp8", note_eg="which build this is", library=_lib.LIB_OVERRIDE or "in-tree")
    legs = bench.legs
    m, ths, prompts = bench.model()
    # the RoPE table has block_size rows and a prompt pass indexes it by position: a long-context run raises the synthetic
    # architecture's 2048 to Llama-2's 4096, as bench.py's value_at_context does, and nothing runs past it
    if bench.max_seq > 2048:
        m.config.block_size = max(m.config.block_size, 4096)
    if bench.max_seq + 8 > m.config.block_size:
        raise SystemExit(f"--pos {bench.a.pos} + --steps {bench.a.steps} needs {bench.max_seq} cache rows: more than the context of "
                         f"{m.config.block_size}")
    if {"1", "3", "4"} & set(legs):
        leg_pair(bench, m, ths, prompts, 8, legs)
    if {"2", "3"} & set(legs):
        leg_pair(bench, m, ths, prompts, 1, legs)
    bench.close()


if __name__ == "__main__":
    main()
