"""What per-request sampling costs: the decode step with it off, on at the defaults (top_p = 1, min_p = 0: the fused top-k sampler's
tokens) and on with top-p and min-p active on a synthetic model, and the sampling launch by itself.

    python scripts/sampling_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/per_request_sampling_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (off, defaults, nucleus, off, defaults,
nucleus: every setting is run twice, and the spread between a setting's two runs is the noise a difference has to beat), and every
timed window starts from the same token, positions and draw counters.

  leg 1  DecodeEngine: ms per step (one replay = the forward pass and the sampler / the sampling launch)
  leg 2  SlotDecodeEngine at B = 8, all slots active: ms per step (B slot samplers / one sampling launch of B rows, retire)
  leg 3  the launch alone, vocab 32000 and 128256, B = 1 and 8: a graph of --chain consecutive launches on the same rows — us per
         launch, including the same-stream launch boundary — for teal_sample_rows (top-k only; top-k + top-p + min-p; top-p alone)
         against the B teal_sample_topk_slot launches it replaces

--legs 1,2 --settings off runs on a tree without the feature too (the parent commit's step, for the off leg's comparison).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from teal_amd import _lib, runtime  # noqa: E402
from teal_amd.gpt_fast import generate as G  # noqa: E402
from teal_amd.gpt_fast.engine import DecodeEngine  # noqa: E402

T, TOP_K = 0.8, 200
SETTINGS = {"defaults": (T, TOP_K, 1.0, 0.0), "nucleus": (T, TOP_K, 0.9, 0.02)}


def replay_ms(g, steps, reset):
    """ms per replay over `steps` replays from the state reset() restores, after 3 warm replays from the same state"""
    reset()
    for _ in range(3):
        g.replay()
    reset()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with runtime.graph_capture(g):
        fn()
    return g


def leg_engine(name, eng, rows, settings, steps, graph_of, state, emit):
    saved = [t.clone() for t in state]

    def reset():
        for t, v in zip(state, saved):
            t.copy_(v)

    for rnd in (1, 2):
        for key in settings:
            if key != "off" or hasattr(eng, "set_sampling_params"):
                eng.set_sampling_params(key != "off")
            if key != "off":
                for r in range(rows):
                    eng.set_slot_sampling(r, *SETTINGS[key])
            ms = replay_ms(graph_of(), steps, reset)
            emit({"leg": name, "sampling": key, "run": rnd, "ms_per_step": round(ms, 4)})


def leg_launch(V, dt, chain, steps, emit):
    from teal_amd.gpt_fast.sampling import check_sampling, row_words
    L = _lib.load()
    code, dev = runtime.dtype_code(dt), "cuda"
    g = torch.Generator(device=dev).manual_seed(V)
    logits = (torch.randn(8, V, device=dev, generator=g) * 3.0).to(dt)
    state = torch.tensor([[1234 + r, 0] for r in range(8)], dtype=torch.int64, device=dev)
    tok = torch.zeros(8, dtype=torch.int32, device=dev)
    pos = torch.zeros(8, dtype=torch.int32, device=dev)
    kept = torch.zeros(8, dtype=torch.int32, device=dev)
    active = torch.tensor([255], dtype=torch.int32, device=dev)
    ws = runtime.new_workspace(64, 64)
    saved = state.clone()

    def rows(B, setting):
        params = torch.stack([row_words(check_sampling(*setting))] * 8).to(dev)

        def fn():
            st = runtime.stream_ptr()  # (read here: the capture runs on a stream of its own)
            for _ in range(chain):
                _lib.check(L.teal_sample_rows(logits.data_ptr(), V, V, code, B, params.data_ptr(), state.data_ptr(), tok.data_ptr(),
                                              pos.data_ptr(), None, 0, kept.data_ptr(), active.data_ptr(), 0, st), "teal_sample_rows")
        return fn, params

    def slots(B):
        def fn():
            st = runtime.stream_ptr()
            for _ in range(chain):
                for b in range(B):
                    _lib.check(L.teal_sample_topk_slot(logits[b].data_ptr(), V, code, TOP_K, T, state[b].data_ptr(), tok[b:].data_ptr(),
                                                       pos[b:].data_ptr(), None, 0, ws.data_ptr(), ws.numel() * 4, active.data_ptr(), b, st),
                               "teal_sample_topk_slot")
        return fn, None

    runs = []
    for B in (1, 8):
        runs.append((f"{B} x teal_sample_topk_slot (top_k {TOP_K})", B) + slots(B))
        runs.append((f"teal_sample_rows top_k {TOP_K}", B) + rows(B, (T, TOP_K, 1.0, 0.0)))
        runs.append((f"teal_sample_rows top_k {TOP_K} top_p 0.9 min_p 0.02", B) + rows(B, (T, TOP_K, 0.9, 0.02)))
        runs.append(("teal_sample_rows top_p 0.9 alone", B) + rows(B, (T, 0, 0.9, 0.0)))
    graphs = [(what, B, capture(fn), keep) for what, B, fn, keep in runs]
    for rnd in (1, 2):
        for what, B, gr, _ in graphs:
            ms = replay_ms(gr, steps, lambda: state.copy_(saved))
            emit({"leg": "launch", "vocab": V, "what": what, "B": B, "run": rnd, "us_per_step_of_B_rows": round(ms * 1e3 / chain, 2)})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--synthetic", default="7B")
    p.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--sparsity", type=float, default=0.5)
    p.add_argument("--n_layer", type=int, default=None)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--pos", type=int, default=32, help="position of the first timed step")
    p.add_argument("--chain", type=int, default=20, help="leg 3: launches per graph")
    p.add_argument("--legs", default="1,2,3")
    p.add_argument("--settings", default="off,defaults,nucleus")
    p.add_argument("--note", default="", help="a line for the head of the record (e.g. which tree this is)")
    p.add_argument("--out", default=None, help="also append the record to this file")
    a = p.parse_args()
    runtime.init()
    dev, dt = "cuda", {"fp16": torch.float16, "bf16": torch.bfloat16}[a.precision]
    legs, settings = a.legs.split(","), a.settings.split(",")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    emit({"model": a.synthetic, "n_layer": a.n_layer, "precision": a.precision, "sparsity": a.sparsity, "steps": a.steps, "pos": a.pos,
          "chain": a.chain, "device": torch.cuda.get_device_name(0), "note": a.note})
    if "1" in legs or "2" in legs:
        m = G.build_synthetic_model(a.synthetic, dev, dt, n_layer=a.n_layer)
        ths = G.apply_sparsity(m, sparsity=a.sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
        V = m.config.vocab_size
        max_seq = a.pos + a.steps + 16
        g = torch.Generator(device=dev).manual_seed(0)
        prompts = [torch.randint(0, V, (a.pos - s,), generator=torch.Generator().manual_seed(s)).tolist() for s in range(8)]
    if "1" in legs:
        m.max_seq_length, m.max_batch_size = -1, -1
        m.setup_caches(max_batch_size=1, max_seq_length=max_seq)
        eng = DecodeEngine(m, ths)
        eng.tok_buf.copy_(torch.randint(0, V, (1, 1), device=dev, generator=g))
        eng.pos_buf.fill_(a.pos)
        eng.rng_state.copy_(torch.tensor([1234, 0], dtype=torch.int64))
        leg_engine("DecodeEngine", eng, 1, settings, a.steps, lambda: eng.capture_loop(T, TOP_K), [eng.tok_buf, eng.pos_buf, eng.rng_state], emit)
        del eng
    if "2" in legs:
        from teal_amd.gpt_fast.batched import SlotDecodeEngine
        B = 8
        m.max_seq_length, m.max_batch_size = -1, -1
        m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
        eng = SlotDecodeEngine(m, ths, B)
        for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
            eng.admit(s, prompts[s], max_seq, None, 1234 + s, T, TOP_K)
        leg_engine("SlotDecodeEngine B=8", eng, B, settings, a.steps, lambda: eng.capture(T, TOP_K),
                   [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state], emit)
        assert eng.read_state()[0] == (1 << B) - 1, "a slot retired inside the timed window"
        del eng
    if "3" in legs:
        for V in (32000, 128256):
            leg_launch(V, dt, a.chain, a.steps, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
