"""The stream attention body against the chunked body (SlotDecodeEngine(attention=)), on a synthetic model with the slots admitted
at about --pos cached rows, for both cache formats.  A sibling of scripts/kv_fp8_bench.py with the same protocol: HIP events over
hipGraph replays, the two bodies alternated in one process, every setting run twice — the spread between a setting's two runs is
the resolution of the comparison — and every timed window started from the same tokens, positions, draw counters and slot state.

    python scripts/stream_attention_bench.py --synthetic 7B --precision fp16 --pos 3800 --out profiles/stream_attention_bench_7b_fp16.txt
    python scripts/stream_attention_bench.py --synthetic llama-3-8b --precision bf16 --pos 3800 ...      (grouped-query: hq = 4)

  leg 1  the attention launch of layer 0 alone, at B = 8 and with one slot: a graph of --chain launches, ms per launch, and the
         achieved TB/s over the K / V bytes the launch has to read (cached rows x n_kv x hd x 2 tensors, the fp8 scales included)
  leg 2  the step, at B = 8 and with one slot: ms per step
  leg 3  teal_kv8_quantize_rows over a prompt's rows, the card's streaming rate in the same run (bytes read + written)
"""
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SlotDecodeEngine

T, TOP_K = 0.8, 200
FORMATS = ("model", "fp8")


def build(bench, m, ths, prompts, B, fmt, body):
    eng = SlotDecodeEngine(m, ths, B, attention=body, **({} if fmt == "model" else {"kv_cache": fmt}))
    for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
        eng.admit(s, prompts[s], bench.max_seq, None, 1234 + s, T, TOP_K)
    state = [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state]
    saved = [t.clone() for t in state]

    def reset():
        for t, v in zip(state, saved):
            t.copy_(v)

    g = eng.capture(T, TOP_K)
    reset()
    at, ns = m.layers[0].attention, eng.splits[0][0]
    chain = capture(lambda: [eng._attention(at, eng.slabs[0], ns, runtime.stream_ptr()) for _ in range(bench.a.chain)])
    cfg = m.config
    rows = sum(eng.pos_buf[:B].tolist())
    kv_bytes = rows * cfg.n_local_heads * 2 * (cfg.head_dim * (2 if fmt == "model" else 1) + (0 if fmt == "model" else 4))
    return {"eng": eng, "step": g, "chain": chain, "reset": reset, "kv_bytes": kv_bytes, "cached_rows": rows}


def leg_group(bench, m, ths, prompts, B, fmt):
    # (the two bodies of a format share the model's caches: both store the same words into the same rows)
    bench.caches(m, B if fmt == "model" else 1)
    built = {body: build(bench, m, ths, prompts, B, fmt, body) for body in bench.settings}
    if "1" in bench.legs:
        for rnd, body in bench.rounds():
            b = built[body]
            ms = replay_ms(b["chain"], max(10, bench.a.steps // 4), b["reset"]) / bench.a.chain
            bench.emit({"leg": f"attention launch alone, B={B}", "kv_cache": fmt, "attention": body, "run": rnd, "ms_per_launch": round(ms, 5),
                        "cached_rows": b["cached_rows"], "kv_MB": round(b["kv_bytes"] / 1e6, 2), "TB_per_s": round(b["kv_bytes"] / ms / 1e9, 3)})
    if "2" in bench.legs:
        for rnd, body in bench.rounds():
            b = built[body]
            ms = replay_ms(b["step"], bench.a.steps, b["reset"])
            assert b["eng"].read_state()[SLOT_ACTIVE] == (1 << B) - 1, "a slot retired inside the timed window"
            bench.emit({"leg": f"SlotDecodeEngine B={B}", "kv_cache": fmt, "attention": body, "run": rnd, "ms_per_step": round(ms, 4)})
    if "3" in bench.legs and fmt == "fp8" and B == 8:
        eng, rows, cfg = built[bench.settings[0]]["eng"], len(prompts[7]), m.config
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            eng._quantize_rows(7, rows)
        e0.record()
        for _ in range(20):
            eng._quantize_rows(7, rows)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / 20
        nbytes = rows * 2 * len(m.layers) * cfg.n_local_heads * (3 * cfg.head_dim + 4)
        bench.emit({"leg": "teal_kv8_quantize_rows alone", "rows": rows, "ms_per_launch": round(ms, 5), "MB": round(nbytes / 1e6, 2),
                    "TB_per_s": round(nbytes / ms / 1e9, 3)})


def main():
    bench = FeatureBench("chunked,stream", note_eg="which build this is", library=_lib.LIB_OVERRIDE or "in-tree")
    m, ths, prompts = bench.model()
    if bench.max_seq > 2048:  # (the RoPE table has block_size rows: as scripts/kv_fp8_bench.py)
        m.config.block_size = max(m.config.block_size, 4096)
    if bench.max_seq + 8 > m.config.block_size:
        raise SystemExit(f"--pos {bench.a.pos} + --steps {bench.a.steps} needs {bench.max_seq} cache rows: more than the context of "
                         f"{m.config.block_size}")
    for B in (8, 1):
        for fmt in FORMATS:
            leg_group(bench, m, ths, prompts, B, fmt)
    bench.close()


if __name__ == "__main__":
    main()
