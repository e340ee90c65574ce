"""What the per-request logit processors cost: the decode step with them off, on at identity parameters and on with all four
controls on a synthetic model, and the processor launch by itself.

    python scripts/logit_processors_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/logit_processors_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (off, identity, all, off, identity,
all: every setting is run twice, and the spread between a setting's two runs is the noise a difference has to beat), and every
timed window starts from the same token, positions, draw counters and processor state.

  leg 1  DecodeEngine: ms per step (one replay = the forward pass, with processors on the processor launch, and the sampler)
  leg 2  SlotDecodeEngine at B = 8, all slots active: ms per step (one processor launch of B rows, B samplers, retire)
  leg 3  the launch alone, vocab 32000 and 128256: a graph of --chain consecutive launches on the same rows — us per launch,
         including the same-stream launch boundary — for teal_logit_adjust at B = 1 and 8, with and without a bias row

--legs 1 --settings off runs on a tree without the feature too (the parent commit's step, for the off leg's comparison).
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

ALL = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, logit_bias={"3": 4.0, "100": -100.0, "2000": 1.5})


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


def leg_engine(name, eng, rows, prompts, settings, steps, graph_of, state, emit):
    saved = [t.clone() for t in state]
    for rnd in (1, 2):
        for key in settings:
            if key != "off" or hasattr(eng, "set_logit_processors"):
                eng.set_logit_processors(key != "off")
            if key != "off":
                for r in range(rows):
                    eng.set_slot_processors(r, prompts[r], **(ALL if key == "all" else {}))
            full = list(state) + ([eng._proc.state] if key != "off" else [])
            keep = saved + ([eng._proc.state.clone()] if key != "off" else [])

            def reset():
                for t, v in zip(full, keep):
                    t.copy_(v)

            ms = replay_ms(graph_of(), steps, reset)
            emit({"leg": name, "processors": key, "run": rnd, "ms_per_step": round(ms, 4)})


def leg_launch(V, dt, chain, steps, emit):
    L = _lib.load()
    code, dev = runtime.dtype_code(dt), "cuda"
    g = torch.Generator(device=dev).manual_seed(V)
    logits = (torch.randn(8, V, device=dev, generator=g) * 4.0).to(dt)
    out = torch.zeros_like(logits)
    bias = (torch.randn(8, V, device=dev, generator=g) * (torch.rand(8, V, device=dev, generator=g) < 0.01)).to(dt)
    state = (torch.randint(0, 4, (8, V), device=dev, generator=g) * (torch.rand(8, V, device=dev, generator=g) < 0.05)).to(torch.int32)
    params = torch.tensor([[1.3, 0.5, 0.2, 0.0]] * 8, dtype=torch.float32, device=dev)
    tok = torch.randint(0, V, (8,), device=dev, generator=g).to(torch.int32)
    saved = state.clone()

    def adjust(B, with_bias):
        st = runtime.stream_ptr()
        for _ in range(chain):
            _lib.check(L.teal_logit_adjust(logits.data_ptr(), V, V, code, B, tok.data_ptr(), 1, state.data_ptr(), params.data_ptr(),
                                           bias.data_ptr() if with_bias else None, out.data_ptr(), V, None, 0, st), "teal_logit_adjust")

    runs = [(f"logit_adjust {'with' if wb else 'no'} bias", lambda B=B, wb=wb: adjust(B, wb), B, wb) for B in (1, 8) for wb in (True, False)]
    graphs = [(what, capture(fn), B, wb) for what, fn, B, wb in runs]
    es = logits.element_size()
    for rnd in (1, 2):
        for what, gr, B, wb in graphs:
            ms = replay_ms(gr, steps, lambda: state.copy_(saved))
            nbytes = B * V * (2 * es + 4 + (es if wb else 0))  # logits in, out, state words, bias
            emit({"leg": "launch", "vocab": V, "what": what, "B": B, "run": rnd, "us_per_launch": round(ms * 1e3 / chain, 2),
                  "bytes_per_launch": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3 / chain) / 1e9, 1)})


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
    p.add_argument("--settings", default="off,identity,all")
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
        leg_engine("DecodeEngine", eng, 1, prompts, settings, a.steps, lambda: eng.capture_loop(0.8, 200),
                   [eng.tok_buf, eng.pos_buf, eng.rng_state], emit)
        del eng
    if "2" in legs:
        from teal_amd.gpt_fast.batched import SlotDecodeEngine
        B = 8
        m.max_seq_length, m.max_batch_size = -1, -1
        m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
        eng = SlotDecodeEngine(m, ths, B)
        for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
            eng.admit(s, prompts[s], max_seq, None, 1234 + s)
        leg_engine("SlotDecodeEngine B=8", eng, B, prompts, settings, a.steps, lambda: eng.capture(0.8, 200),
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
