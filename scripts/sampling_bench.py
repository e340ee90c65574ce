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
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime

T, TOP_K = 0.8, 200
SETTINGS = {"defaults": (T, TOP_K, 1.0, 0.0), "nucleus": (T, TOP_K, 0.9, 0.02)}


def leg_engine(bench, name, eng, rows, graph_of, state):
    saved = [t.clone() for t in state]

    def reset():
        for t, v in zip(state, saved):
            t.copy_(v)

    for rnd, key in bench.rounds():
        if key != "off" or hasattr(eng, "set_sampling_params"):
            eng.set_sampling_params(key != "off")
        if key != "off":
            for r in range(rows):
                eng.set_slot_sampling(r, *SETTINGS[key])
        ms = replay_ms(graph_of(), bench.a.steps, reset)
        bench.emit({"leg": name, "sampling": key, "run": rnd, "ms_per_step": round(ms, 4)})


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
    bench = FeatureBench("off,defaults,nucleus")
    a, legs = bench.a, bench.legs
    if "1" in legs or "2" in legs:
        m, ths, prompts = bench.model()
    if "1" in legs:
        eng, state = bench.decode_engine(m, ths)
        leg_engine(bench, "DecodeEngine", eng, 1, lambda: eng.capture_loop(T, TOP_K), state)
        del eng
    if "2" in legs:
        eng, state = bench.slot_engine(m, ths, prompts)  # (admitted at admit's own defaults: T and TOP_K)
        leg_engine(bench, "SlotDecodeEngine B=8", eng, eng.B, lambda: eng.capture(T, TOP_K), state)
        assert eng.read_state()[0] == (1 << eng.B) - 1, "a slot retired inside the timed window"
        del eng
    if "3" in legs:
        for V in (32000, 128256):
            leg_launch(V, bench.dt, a.chain, a.steps, bench.emit)
    bench.close()


if __name__ == "__main__":
    main()
