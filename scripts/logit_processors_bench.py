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
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime

ALL = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, logit_bias={"3": 4.0, "100": -100.0, "2000": 1.5})


def leg_engine(bench, name, eng, rows, prompts, graph_of, state):
    saved = [t.clone() for t in state]
    for rnd, key in bench.rounds():
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

        ms = replay_ms(graph_of(), bench.a.steps, reset)
        bench.emit({"leg": name, "processors": key, "run": rnd, "ms_per_step": round(ms, 4)})


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
    bench = FeatureBench("off,identity,all")
    a, legs = bench.a, bench.legs
    if "1" in legs or "2" in legs:
        m, ths, prompts = bench.model()
    if "1" in legs:
        eng, state = bench.decode_engine(m, ths)
        leg_engine(bench, "DecodeEngine", eng, 1, prompts, lambda: eng.capture_loop(0.8, 200), state)
        del eng
    if "2" in legs:
        eng, state = bench.slot_engine(m, ths, prompts)
        leg_engine(bench, "SlotDecodeEngine B=8", eng, eng.B, prompts, lambda: eng.capture(0.8, 200), state)
        assert eng.read_state()[0] == (1 << eng.B) - 1, "a slot retired inside the timed window"
        del eng
    if "3" in legs:
        for V in (32000, 128256):
            leg_launch(V, bench.dt, a.chain, a.steps, bench.emit)
    bench.close()


if __name__ == "__main__":
    main()
