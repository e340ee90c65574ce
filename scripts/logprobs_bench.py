"""What token log-probabilities cost: the decode step with logprobs off, 0 and 5 on a synthetic model, and the logprob launch by
itself next to the sampler launch.

    python scripts/logprobs_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/logprobs_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (off, 0, 5, off, 0, 5: every
setting is run twice, and the spread between a setting's two runs is the noise a difference has to beat), and every timed window
starts from the same token, positions and draw counters.

  leg 1  DecodeEngine: ms per step (one replay = the forward pass, the sampler, and with logprobs on the logprob launch)
  leg 2  SlotDecodeEngine at B = 8, all slots active: ms per step (B samplers, one logprob launch of B rows, retire)
  leg 3  the launches alone, vocab 32000 and 128256: a graph of --chain consecutive launches on the same rows — us per launch,
         including the same-stream launch boundary — for the sampler (top-k 200, temperature 0.8, prepared workspace: what the
         engines launch) and for teal_token_logprobs at top_n = 0 and 5, B = 1 and 8

--legs 1 --settings off runs on a tree without the feature too (the parent commit's step, for the off leg's comparison).
"""
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime

SETTINGS = {"off": None, "0": 0, "5": 5}


def leg_engine(bench, name, eng, graph_of, state):
    saved = [t.clone() for t in state]

    def reset():
        for t, v in zip(state, saved):
            t.copy_(v)

    for rnd, key in bench.rounds():
        if key != "off" or hasattr(eng, "set_logprobs"):
            eng.set_logprobs(SETTINGS[key])
        reset()
        ms = replay_ms(graph_of(), bench.a.steps, reset)
        bench.emit({"leg": name, "logprobs": key, "run": rnd, "ms_per_step": round(ms, 4)})


def leg_launches(V, dt, chain, steps, emit):
    L = _lib.load()
    code, dev = runtime.dtype_code(dt), "cuda"
    g = torch.Generator(device=dev).manual_seed(V)
    logits = (torch.randn(8, V, device=dev, generator=g) * 4.0).to(dt)
    ws = runtime.new_workspace(4096, V)
    tok = torch.zeros(8, dtype=torch.int32, device=dev)
    rng = torch.tensor([[1234 + b, 1] for b in range(8)], dtype=torch.int64, device=dev)
    lp = torch.zeros(8, 4, device=dev)
    ids, tlp = torch.zeros(8, 4, 8, dtype=torch.int32, device=dev), torch.zeros(8, 4, 8, device=dev)
    saved = rng.clone()

    def sampler(B):
        st = runtime.stream_ptr()
        for _ in range(chain):
            for b in range(B):
                _lib.check(L.teal_sample_topk_ws(logits[b].data_ptr(), V, code, 200, 0.8, rng[b].data_ptr(), tok[b:].data_ptr(), None, None, 0,
                                                 ws.data_ptr(), ws.numel() * 4, st), "teal_sample_topk_ws")

    def logprob(B, n):
        st = runtime.stream_ptr()
        for _ in range(chain):
            _lib.check(L.teal_token_logprobs(logits.data_ptr(), V, V, code, B, tok.data_ptr(), rng.data_ptr(), lp.data_ptr(), 4, n,
                                             ids.data_ptr() if n else None, tlp.data_ptr() if n else None, None, 0, st), "teal_token_logprobs")

    runs = [("sampler x B", lambda B=B: sampler(B), B, B) for B in (1, 8)] + \
           [(f"logprobs top_n={n}", lambda B=B, n=n: logprob(B, n), B, 1) for B in (1, 8) for n in (0, 5)]
    graphs = [(what, capture(fn), B, per) for what, fn, B, per in runs]
    for rnd in (1, 2):
        for what, gr, B, per in graphs:
            ms = replay_ms(gr, steps, lambda: rng.copy_(saved))
            emit({"leg": "launch", "vocab": V, "what": what, "B": B, "run": rnd, "launches_per_step": per,
                  "us_per_step": round(ms * 1e3 / chain, 2), "us_per_launch": round(ms * 1e3 / chain / per, 2)})


def main():
    bench = FeatureBench("off,0,5")
    a, legs = bench.a, bench.legs
    if "1" in legs or "2" in legs:
        m, ths, prompts = bench.model()
    if "1" in legs:
        eng, state = bench.decode_engine(m, ths)
        leg_engine(bench, "DecodeEngine", eng, lambda: eng.capture_loop(0.8, 200), state)
        del eng
    if "2" in legs:
        eng, state = bench.slot_engine(m, ths, prompts)
        leg_engine(bench, "SlotDecodeEngine B=8", eng, lambda: eng.capture(0.8, 200), state)
        assert eng.read_state()[0] == (1 << eng.B) - 1, "a slot retired inside the timed window"
        del eng
    if "3" in legs:
        for V in (32000, 128256):
            leg_launches(V, bench.dt, a.chain, a.steps, bench.emit)
    bench.close()


if __name__ == "__main__":
    main()
