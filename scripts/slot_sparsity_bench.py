"""What per-request sparsity costs: the continuous-batching step with the feature off, on with every slot at the engine's own level,
and a batch that mixes levels, on a synthetic model.

    python scripts/slot_sparsity_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/per_request_sparsity_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (every setting is run twice, and the
spread between a setting's two runs is the noise a difference has to beat), and every timed window starts from the same tokens,
positions, draw counters and slot state: the slots are admitted afresh for every window.

  leg 1  SlotDecodeEngine at B = 8, all slots active: ms per step, settings off | on (every column at the engine's own thresholds)
  leg 2  SlotDecodeEngine with one slot: ms per step, the same settings
  leg 3  SlotDecodeEngine with four slots, feature on: all four at --sparsity, all four at level 0 (every row kept), two and two —
         ms per step and the fraction of rows the union kept, per projection

--legs 1,2 --settings off runs on a library without the feature too (TEAL_LIB_PATH: the parent commit's build, for the off leg's
comparison in alternating processes).
"""
from _feature_bench import FeatureBench, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SlotDecodeEngine
from teal_amd.gpt_fast.score import dense_thresholds

T, TOP_K = 0.8, 200


def window(bench, eng, B, prompts, on, levels=None):
    """the slots admitted afresh (levels: per slot thresholds or None), then one timed window -> ms per step"""
    eng.slot_state[SLOT_ACTIVE:SLOT_ACTIVE + 1].zero_()  # (every slot dropped: the feature is switched on an idle engine only)
    if on or eng.tau_table is not None:
        eng.set_slot_sparsity(on)
    for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
        kw = {"thresholds": levels[s]} if levels and levels[s] is not None else {}
        eng.admit(s, prompts[s], bench.max_seq, None, 1234 + s, T, TOP_K, **kw)
    state = [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state]
    saved = [t.clone() for t in state]

    def reset():
        for t, v in zip(state, saved):
            t.copy_(v)

    ms = replay_ms(eng.capture(T, TOP_K), bench.a.steps, reset)
    assert eng.read_state()[SLOT_ACTIVE] == (1 << B) - 1, "a slot retired inside the timed window"
    return ms


def leg_engine(bench, name, m, ths, B, prompts):
    bench.caches(m, B)
    eng = SlotDecodeEngine(m, ths, B)
    for rnd, key in bench.rounds():
        ms = window(bench, eng, B, prompts, key == "on")
        bench.emit({"leg": name, "slot_sparsity": key, "run": rnd, "ms_per_step": round(ms, 4)})
    del eng


def leg_mixed(bench, m, ths, prompts):
    B, dense = 4, dense_thresholds(ths)
    bench.caches(m, B)
    eng = SlotDecodeEngine(m, ths, B)
    mixes = (("all at the level", [None] * 4), ("all at level 0", [dense] * 4), ("two and two", [None, dense, None, dense]))
    for rnd in (1, 2):
        for what, levels in mixes:
            ms = window(bench, eng, B, prompts, True, levels)
            union = {p: round(v["union"], 4) for p, v in eng.kept_fractions().items()}
            kept = {p: [round(x, 3) for x in v] for p, v in eng.kept_by_slot().items() if p in ("q", "down")}
            bench.emit({"leg": "SlotDecodeEngine B=4, feature on", "levels": what, "run": rnd, "ms_per_step": round(ms, 4),
                        "union_kept": union, "kept_by_slot": kept})
    del eng


def main():
    bench = FeatureBench("off,on", note_eg="which build this is", library=_lib.LIB_OVERRIDE or "in-tree")
    legs = bench.legs
    m, ths, prompts = bench.model()
    for leg, B in (("1", 8), ("2", 1)):
        if leg in legs:
            leg_engine(bench, f"SlotDecodeEngine B={B}", m, ths, B, prompts)
    if "3" in legs:
        leg_mixed(bench, m, ths, prompts)
    bench.close()


if __name__ == "__main__":
    main()
