"""What per-request stop conditions cost: the continuous-batching step with the feature off, on with empty stop tables and on with
full tables (16 stop ids and 8 stop sequences of 8 tokens per slot, none of which ever matches) on a synthetic model, and the retire
launch by itself.

    python scripts/stop_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/stop_conditions_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (off, empty, full, off, empty, full:
every setting is run twice, and the spread between a setting's two runs is the noise a difference has to beat), and every timed
window starts from the same tokens, positions, draw counters and slot state: the slots are admitted afresh for every window.

  leg 1  SlotDecodeEngine at B = 8, all slots active: ms per step (one replay = the forward pass, B slot samplers, the retire launch)
  leg 2  SlotDecodeEngine with one slot: ms per step
  leg 3  the launch alone at B = 8: a graph of --chain consecutive launches on the same slot state — us per launch, including the
         same-stream launch boundary — for teal_batched_retire_stops (empty tables; full tables) against teal_batched_retire

The full tables hold ids the window never draws (found by running the window once with the feature off), so no slot retires and
every window does the same work; a sequence's eight compares are issued whether or not its last token matches.

--legs 1,2 --settings off runs on a library without the feature too (TEAL_LIB_PATH: the parent commit's build, for the off leg's
comparison in alternating processes).
"""
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_WORDS, SlotDecodeEngine

T, TOP_K = 0.8, 200


def full_tables(unused):
    """16 stop ids and 8 sequences of 8 tokens, all out of ids the window never draws"""
    ids = unused[:16]
    return dict(stop_token_ids=ids, stop_sequences=[[ids[q]] * 8 for q in range(8)])


def leg_engine(bench, name, m, ths, B, prompts):
    bench.caches(m, B)
    eng = SlotDecodeEngine(m, ths, B)
    V, max_seq, settings, steps = m.config.vocab_size, bench.max_seq, bench.settings, bench.a.steps

    def window(key, stops):
        """the slots admitted afresh under `key`, then one timed window"""
        eng.slot_state[SLOT_ACTIVE:SLOT_ACTIVE + 1].zero_()  # (every slot dropped: the feature is switched on an idle engine only)
        if hasattr(eng, "set_stop_conditions"):
            eng.set_stop_conditions(key != "off")
        for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
            eng.admit(s, prompts[s], max_seq, None, 1234 + s, T, TOP_K, **stops)
        state = [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state] + ([eng.stop_table] if key != "off" else [])
        saved = [t.clone() for t in state]

        def reset():
            for t, v in zip(state, saved):
                t.copy_(v)

        ms = replay_ms(eng.capture(T, TOP_K), steps, reset)
        assert eng.read_state()[SLOT_ACTIVE] == (1 << B) - 1, "a slot retired inside the timed window"
        return ms

    unused = []
    if "full" in settings:  # the window once with the feature off: what it draws
        window("off", {})
        drawn = set(eng.history[:, :steps + 8].flatten().tolist())
        unused = [t for t in range(V - 1, -1, -1) if t not in drawn][:16]
    for rnd, key in bench.rounds():
        ms = window(key, full_tables(unused) if key == "full" else {})
        bench.emit({"leg": name, "stop_conditions": key, "run": rnd, "ms_per_step": round(ms, 4)})
    del eng


def leg_launch(chain, steps, emit):
    from teal_amd.gpt_fast.stopping import StopConditions
    L = _lib.load()
    dev, B, max_seq, V = "cuda", 8, 1 << 20, 32000
    stride = 16 + (steps + 3) * chain + 8  # a slot's n stays inside its history row over a whole window
    g = torch.Generator(device=dev).manual_seed(7)
    hist = torch.randint(0, V - 64, (B, stride), device=dev, generator=g, dtype=torch.int32)
    tok = hist[:, 0].clone()
    pos = torch.full((B,), 40, dtype=torch.int32, device=dev)
    state = torch.zeros(SLOT_WORDS, dtype=torch.int32, device=dev)
    state[0], state[8:16], state[16:24], state[24:32], state[32:40] = 255, 1 << 30, 16, -1, -1
    saved = state.clone()
    tables = {"empty": StopConditions(B, V, dev), "full": StopConditions(B, V, dev)}
    for s in range(B):
        tables["full"].set_row(s, **full_tables(list(range(V - 1, V - 17, -1))))  # (the history holds ids below V - 64)

    def plain():
        st = runtime.stream_ptr()  # (read here: the capture runs on a stream of its own)
        for _ in range(chain):
            _lib.check(L.teal_batched_retire(state.data_ptr(), tok.data_ptr(), pos.data_ptr(), B, 255, max_seq, 1, st), "teal_batched_retire")

    def stops(which):
        def fn():
            st = runtime.stream_ptr()
            for _ in range(chain):
                tables[which].launch(state.data_ptr(), tok, pos, hist, B, 255, max_seq, True, st=st)
        return fn

    runs = [("teal_batched_retire", plain), ("teal_batched_retire_stops, empty tables", stops("empty")),
            ("teal_batched_retire_stops, 16 ids + 8 sequences of 8", stops("full"))]
    graphs = [(what, capture(fn)) for what, fn in runs]
    for rnd in (1, 2):
        for what, gr in graphs:
            ms = replay_ms(gr, steps, lambda: state.copy_(saved))
            assert int(state[0]) == 255, "a slot retired inside the timed window"
            emit({"leg": "launch", "what": what, "B": B, "run": rnd, "us_per_launch": round(ms * 1e3 / chain, 2)})


def main():
    bench = FeatureBench("off,empty,full", note_eg="which build this is", library=_lib.LIB_OVERRIDE or "in-tree")
    a, legs = bench.a, bench.legs
    if "1" in legs or "2" in legs:
        m, ths, prompts = bench.model()
        for leg, B in (("1", 8), ("2", 1)):
            if leg in legs:
                leg_engine(bench, f"SlotDecodeEngine B={B}", m, ths, B, prompts)
    if "3" in legs:
        leg_launch(a.chain, a.steps, bench.emit)
    bench.close()


if __name__ == "__main__":
    main()
