"""What teacher-forced requests cost: the continuous-batching step with the feature off, on with no forced row and on with every
slot forced on a synthetic model, the forcing launch by itself next to the retire launch, and batched scoring against the
single-stream scorer.

    python scripts/forced_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/forced_tokens_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (off, none, all, off, none, all: every
setting is run twice, and the spread between a setting's two runs is the noise a difference has to beat), and every timed window
starts from the same tokens, positions, draw counters and slot state: the slots are admitted afresh for every window.

  leg 1  SlotDecodeEngine at B = 8, all slots active: ms per step (one replay = the forward pass, B slot samplers, the forcing launch
         where the feature is on, the retire launch)
  leg 2  SlotDecodeEngine with one slot: ms per step
  leg 3  the launch alone at B = 8: a graph of --chain consecutive launches — us per launch, including the same-stream launch
         boundary — for teal_force_tokens (no forced row; every row forced) against teal_batched_retire in the same process
  leg 4  scoring: 16 windows of 64 random tokens (WINDOWS, WINDOW below) through score.py's two paths on the same model — DecodeEngine.score
         one window at a time, and the same windows as teacher-forced requests of a SlotDecodeEngine with 8 slots — scored tokens
         per second (HIP events around the second of two passes; a batched pass switches its features on afresh, so it holds one
         graph capture and every window's admission), both perplexity pairs, and the mean |difference| of a scored token's
         logprob between the two paths by its place in the window; the relative difference between the batched and the
         single-stream perplexity is reported, not asserted

"all" forces every slot to random token ids for the whole window: a forced row does the launch's second load round and its two
stores, a row without forced tokens stops after the first.

--legs 1,2 --settings off runs on a library without the feature too (TEAL_LIB_PATH: the parent commit's build, for the off leg's
comparison in alternating processes).
"""
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_WORDS, SlotDecodeEngine

T, TOP_K = 0.8, 200
WINDOWS, WINDOW = 16, 64  # leg 4


def leg_engine(bench, name, m, ths, B, prompts):
    bench.caches(m, B)
    eng = SlotDecodeEngine(m, ths, B)
    V, max_seq, steps = m.config.vocab_size, bench.max_seq, bench.a.steps
    g = torch.Generator().manual_seed(11)
    rows = [torch.randint(0, V, (steps + 8,), generator=g).tolist() for _ in range(B)]

    def window(key):
        """the slots admitted afresh under `key`, then one timed window"""
        eng.slot_state[SLOT_ACTIVE:SLOT_ACTIVE + 1].zero_()  # (every slot dropped: the feature is switched on an idle engine only)
        if key != "off":
            eng.set_forced_tokens(True)
        elif eng._frc is not None:
            eng.set_forced_tokens(False)
        for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
            eng.admit(s, prompts[s], max_seq, None, 1234 + s, T, TOP_K, **({"forced_tokens": rows[s]} if key == "all" else {}))
        state = [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state]
        saved = [t.clone() for t in state]

        def reset():
            for t, v in zip(state, saved):
                t.copy_(v)

        ms = replay_ms(eng.capture(T, TOP_K), steps, reset)
        assert eng.read_state()[SLOT_ACTIVE] == (1 << B) - 1, "a slot retired inside the timed window"
        if key == "all":  # the window's last draws were forced ones
            assert eng.read_history(0, steps + 1)[1:] == rows[0][1:steps + 1], "the window outran its forced rows"
        return ms

    for rnd, key in bench.rounds():
        bench.emit({"leg": name, "forced_tokens": key, "run": rnd, "ms_per_step": round(window(key), 4)})
    del eng


def leg_launch(chain, steps, emit):
    from teal_amd.gpt_fast.forcing import ForcedTokens
    L = _lib.load()
    dev, B, max_seq, V = "cuda", 8, 1 << 20, 32000
    hist_len = 64
    g = torch.Generator(device=dev).manual_seed(7)
    tok = torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32)
    pos = torch.full((B,), 40, dtype=torch.int32, device=dev)
    hist = torch.zeros(B, hist_len, dtype=torch.int32, device=dev)
    rng = torch.tensor([[1234 + b, 17 + b] for b in range(B)], dtype=torch.int64).to(dev)  # draw counters inside the forced rows
    state = torch.zeros(SLOT_WORDS, dtype=torch.int32, device=dev)
    state[0], state[8:16], state[16:24], state[24:32], state[32:40] = 255, 1 << 30, 16, -1, -1
    saved = state.clone()
    tables = {"none": ForcedTokens(B, hist_len, V, dev), "all": ForcedTokens(B, hist_len, V, dev)}
    for s in range(B):
        tables["all"].set_row(s, torch.randint(0, V, (hist_len,), generator=torch.Generator().manual_seed(s)).tolist())

    def plain():
        st = runtime.stream_ptr()  # (read here: the capture runs on a stream of its own)
        for _ in range(chain):
            _lib.check(L.teal_batched_retire(state.data_ptr(), tok.data_ptr(), pos.data_ptr(), B, 255, max_seq, 1, st), "teal_batched_retire")

    def force(which):
        def fn():
            st = runtime.stream_ptr()
            for _ in range(chain):
                tables[which].launch(B, rng, tok, hist, hist_len, active=state.data_ptr(), st=st)
        return fn

    runs = [("teal_batched_retire", plain), ("teal_force_tokens, no forced row", force("none")),
            ("teal_force_tokens, every row forced", force("all"))]
    graphs = [(what, capture(fn)) for what, fn in runs]
    for rnd in (1, 2):
        for what, gr in graphs:
            ms = replay_ms(gr, steps, lambda: state.copy_(saved))
            assert int(state[0]) == 255, "a slot retired inside the timed window"
            emit({"leg": "launch", "what": what, "B": B, "run": rnd, "us_per_launch": round(ms * 1e3 / chain, 2)})
    assert tok.tolist() == tables["all"].table[:, 16:24].diagonal().tolist()  # (row b was forced to its entry 16 + b)


def leg_score(bench, m, ths):
    """score.py's two paths over the same windows on the same model: tokens per second and the two perplexity pairs"""
    from teal_amd.gpt_fast import score as S
    from teal_amd.gpt_fast.engine import DecodeEngine
    V = m.config.vocab_size
    g = torch.Generator().manual_seed(5)
    windows = [torch.randint(0, V, (WINDOW,), generator=g).tolist() for _ in range(WINDOWS)]
    n = sum(len(w) - 1 for w in windows)
    dense = S.dense_thresholds(ths)

    kept = []  # the four passes' logprobs: single sparse, single dense, batched sparse, batched dense

    def timed(fn):
        fn()  # (a pass to warm up on)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lps = fn()
        e1.record()
        e1.synchronize()
        kept.append(lps)
        return S.perplexity(lps), n / (e0.elapsed_time(e1) / 1e3)

    m.max_seq_length, m.max_batch_size = -1, -1
    m.setup_caches(max_batch_size=1, max_seq_length=WINDOW)
    G.relayout_for_engine(m)
    eng = DecodeEngine(m, ths)
    ppl1, tps1 = timed(lambda: S.score_windows(eng, windows))
    eng.set_thresholds(dense)
    ppl1d, tps1d = timed(lambda: S.score_windows(eng, windows))
    del eng
    m.max_seq_length, m.max_batch_size = -1, -1
    m.setup_caches(max_batch_size=8, max_seq_length=WINDOW)
    eng = SlotDecodeEngine(m, ths, 8)
    ppl8, tps8 = timed(lambda: S.score_windows_batched(eng, windows))
    del eng
    S.set_module_thresholds(m, dense)
    eng = SlotDecodeEngine(m, dense, 8)
    ppl8d, tps8d = timed(lambda: S.score_windows_batched(eng, windows))
    del eng
    S.set_module_thresholds(m, ths)
    for what, ppl, ppld, tps, tpsd in (("score.py (DecodeEngine.score, one window at a time)", ppl1, ppl1d, tps1, tps1d),
                                       ("score.py --batch_size 8 (teacher-forced requests)", ppl8, ppl8d, tps8, tps8d)):
        bench.emit({"leg": "score", "what": what, "windows": WINDOWS, "window": WINDOW, "scored_tokens": n,
                    "scored_tokens_per_sec": round(tps, 1), "scored_tokens_per_sec_every_row_kept": round(tpsd, 1),
                    "perplexity": round(ppl, 4), "perplexity_every_row_kept": round(ppld, 4)})
    for what, a, b in (("at the sparsity", kept[0], kept[2]), ("every row kept", kept[1], kept[3])):
        # where the two paths part: the mean |difference| of a scored token's logprob by its place in the window (place 0 is the
        # token the batched path scores from its prompt pass; every later one has that pass's K / V row 0 in its context)
        d = (torch.tensor(a, dtype=torch.float64) - torch.tensor(b, dtype=torch.float64)).abs().mean(0)
        bench.emit({"leg": "score", "what": f"mean |logprob difference| by place in the window, {what}",
                    **{f"places {lo}-{hi - 1}": round(float(d[lo:hi].mean()), 5) for lo, hi in ((0, 1), (1, 4), (4, 16), (16, 32), (32, 63))}})
    bench.emit({"leg": "score", "what": "batched against single-stream", "relative_perplexity_difference": round(ppl8 / ppl1 - 1.0, 6),
                "relative_perplexity_difference_every_row_kept": round(ppl8d / ppl1d - 1.0, 6), "speedup": round(tps8 / tps1, 3)})


def main():
    bench = FeatureBench("off,none,all", note_eg="which build this is", library=_lib.LIB_OVERRIDE or "in-tree")
    a, legs = bench.a, bench.legs
    if {"1", "2", "4"} & set(legs):
        m, ths, prompts = bench.model()
        for leg, B in (("1", 8), ("2", 1)):
            if leg in legs:
                leg_engine(bench, f"SlotDecodeEngine B={B}", m, ths, B, prompts)
        if "4" in legs:
            leg_score(bench, m, ths)
    if "3" in legs:
        leg_launch(a.chain, a.steps, bench.emit)
    bench.close()


if __name__ == "__main__":
    main()
