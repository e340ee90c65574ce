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
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from teal_amd import _lib, runtime  # noqa: E402
from teal_amd.gpt_fast import generate as G  # noqa: E402
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_WORDS, SlotDecodeEngine  # noqa: E402

T, TOP_K = 0.8, 200


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


def full_tables(unused):
    """16 stop ids and 8 sequences of 8 tokens, all out of ids the window never draws"""
    ids = unused[:16]
    return dict(stop_token_ids=ids, stop_sequences=[[ids[q]] * 8 for q in range(8)])


def leg_engine(name, m, ths, B, prompts, max_seq, settings, steps, emit):
    eng = SlotDecodeEngine(m, ths, B)
    V = m.config.vocab_size

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
    for rnd in (1, 2):
        for key in settings:
            ms = window(key, full_tables(unused) if key == "full" else {})
            emit({"leg": name, "stop_conditions": key, "run": rnd, "ms_per_step": round(ms, 4)})
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
    p = argparse.ArgumentParser()
    p.add_argument("--synthetic", default="7B")
    p.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--sparsity", type=float, default=0.5)
    p.add_argument("--n_layer", type=int, default=None)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--pos", type=int, default=32, help="position of the first timed step")
    p.add_argument("--chain", type=int, default=20, help="leg 3: launches per graph")
    p.add_argument("--legs", default="1,2,3")
    p.add_argument("--settings", default="off,empty,full")
    p.add_argument("--note", default="", help="a line for the head of the record (e.g. which build this is)")
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
          "chain": a.chain, "device": torch.cuda.get_device_name(0), "library": _lib.LIB_OVERRIDE or "in-tree", "note": a.note})
    if "1" in legs or "2" in legs:
        m = G.build_synthetic_model(a.synthetic, dev, dt, n_layer=a.n_layer)
        ths = G.apply_sparsity(m, sparsity=a.sparsity, hist_path=None, greedy_lookup=None, synthetic=True)
        V = m.config.vocab_size
        max_seq = a.pos + a.steps + 16
        prompts = [torch.randint(0, V, (a.pos - s,), generator=torch.Generator().manual_seed(s)).tolist() for s in range(8)]
        for leg, B in (("1", 8), ("2", 1)):
            if leg in legs:
                m.max_seq_length, m.max_batch_size = -1, -1
                m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
                leg_engine(f"SlotDecodeEngine B={B}", m, ths, B, prompts, max_seq, settings, a.steps, emit)
    if "3" in legs:
        leg_launch(a.chain, a.steps, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
