"""What constrained decoding costs: the continuous-batching step with the feature off, on with every slot unconstrained and on with
every slot on a 64-way trie of 8-token choices, on a synthetic model, and the constrain launch by itself.

    python scripts/constraint_bench.py --synthetic 7B --precision fp16 --sparsity 0.5 --out profiles/constrained_bench_7b_fp16.txt

Everything is timed with HIP events around hipGraph replays.  The settings of a leg alternate (off, free, trie, off, free, trie:
every setting is run twice, and the spread between a setting's two runs is the noise a difference has to beat), and every timed
window starts from the same tokens, positions, draw counters, slot state and trace: the slots are admitted afresh for every window.

  leg 1  SlotDecodeEngine at B = 8, all slots active: ms per step (one replay = the forward pass, the constrain launch when on, B slot
         samplers, the retire launch)
  leg 2  SlotDecodeEngine with one slot: ms per step
  leg 3  the launch alone: a graph of --chain consecutive launches on the same rows — us per launch, including the same-stream launch
         boundary — at vocab 32000 and 128256 with B = 1 and 8, in a sparse state (64 edges), a dense state (default >= 0 with 1000
         banned exceptions) and a state of vocab / 2 listed edges, next to teal_logit_adjust's launch over the same rows; and, at
         B = 1, the fused top-k sampler alone on the model's row and on that row constrained to 64 tokens

The trie: 64 choices of 8 tokens, no two sharing a token; the last edge of every choice leads back to the root, so a window of any
length keeps walking it and no slot retires (a request that ended on its EOS id would leave the window with fewer active slots).

--legs 1,2 --settings off runs on a library without the feature too (TEAL_LIB_PATH: the parent commit's build, for the off leg's
comparison in alternating processes).
"""
import torch

from _feature_bench import FeatureBench, capture, replay_ms  # (puts the repository root on sys.path)
from teal_amd import _lib, runtime
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SlotDecodeEngine

T, TOP_K = 0.8, 200
WAYS, LENGTH = 64, 8


def cyclic_trie(V):
    """64 chains of 8 tokens off the root, each chain's last edge back to the root: the states of a 64-way trie of 8-token choices"""
    from teal_amd.gpt_fast.constraints import Automaton
    step = V // (WAYS * LENGTH)
    states = [{"edges": [], "default": -1, "accept": False}]
    for w in range(WAYS):
        toks = [(w * LENGTH + j) * step for j in range(LENGTH)]
        states[0]["edges"].append((toks[0], len(states)))
        for j in range(1, LENGTH):
            nxt = len(states) + 1 if j < LENGTH - 1 else 0
            states.append({"edges": [(toks[j], nxt)], "default": -1, "accept": False})
    return Automaton(states)


def leg_engine(bench, name, m, ths, B, prompts):
    bench.caches(m, B)
    eng = SlotDecodeEngine(m, ths, B)
    V, max_seq, steps = m.config.vocab_size, bench.max_seq, bench.a.steps

    def window(key):
        """the slots admitted afresh under `key`, then one timed window"""
        eng.slot_state[SLOT_ACTIVE:SLOT_ACTIVE + 1].zero_()  # (every slot dropped: the feature is switched on an idle engine only)
        if hasattr(eng, "set_constraints"):
            eng.set_constraints(key != "off")
        kw = {}
        if key == "trie":
            eng.register_constraint("trie", cyclic_trie(V))
            kw = {"constraint": "trie"}
        for s in range(B):  # prompts of pos - s tokens: the slots sit at different positions, none retires inside a window
            eng.admit(s, prompts[s], max_seq, None, 1234 + s, T, TOP_K, **kw)
        state = [eng.tok_buf, eng.pos_buf, eng.rng_state, eng.slot_state] + ([eng._con.trace] if key != "off" else [])
        saved = [t.clone() for t in state]

        def reset():
            for t, v in zip(state, saved):
                t.copy_(v)

        ms = replay_ms(eng.capture(T, TOP_K), steps, reset)
        assert eng.read_state()[SLOT_ACTIVE] == (1 << B) - 1, "a slot retired inside the timed window"
        if key == "trie":
            assert not any(w & (1 << 30) for w in eng.read_constraint_trace(0, steps + 1)), "a violation bit in the trace"
        return ms

    for rnd, key in bench.rounds():
        bench.emit({"leg": name, "constraints": key, "run": rnd, "ms_per_step": round(window(key), 4)})
    del eng


def leg_launch(chain, steps, dt, emit):
    from teal_amd.gpt_fast.constraints import Automaton, Constraints
    from teal_amd.gpt_fast.logit_processors import LogitProcessors
    dev = "cuda"
    for V in (32000, 128256):
        g = torch.Generator().manual_seed(V)
        perm = torch.randperm(V, generator=g).tolist()
        kinds = {
            "sparse, 64 edges": {"edges": sorted((t, 1) for t in perm[:64]), "default": -1, "accept": True},
            "dense, default >= 0 with 1000 bans": {"edges": sorted((t, -1) for t in perm[:1000]), "default": 1, "accept": True},
            "vocab / 2 listed edges": {"edges": sorted((t, 1) for t in perm[:V // 2]), "default": -1, "accept": True},
        }
        for B in (1, 8):
            logits = (torch.randn(B, V, generator=g) * 3).to(dt).to(dev)
            tok = torch.full((B,), 5, dtype=torch.int32, device=dev)       # the fed token: state 0's one edge, into the measured state
            rng = torch.tensor([[1234 + b, 1] for b in range(B)], dtype=torch.int64, device=dev)  # draw 1: the launch advances, too
            eos = torch.full((B,), -1, dtype=torch.int32, device=dev)
            con = Constraints(B, V, dt, 8, dev, capacity_words=1 << 20)
            for name, st in kinds.items():
                con.register(name, Automaton([{"edges": [(5, 1)], "default": -1, "accept": False}, st]).check(V, None))
            proc = LogitProcessors(B, V, dt, dev)
            runs = [("teal_logit_adjust", None)] + [(f"teal_constrain_logits, {name}", name) for name in kinds] + \
                   [("teal_constrain_logits, unconstrained rows", "")]

            def make(name):
                def fn():
                    st = runtime.stream_ptr()  # (read here: the capture runs on a stream of its own)
                    for _ in range(chain):
                        if name is None:
                            proc.launch(logits, V, B, tok, False, st=st)
                        else:
                            con.launch(logits, V, B, tok, rng, eos.data_ptr(), st=st)
                return fn

            adjust, constrain = capture(make(None)), capture(make(""))
            for rnd in (1, 2):
                for what, name in runs:
                    if name is not None:  # (the table is read on the device: one captured graph serves every kind of state)
                        for r in range(B):
                            con.set_row(r, name or None)
                    ms = replay_ms(adjust if name is None else constrain, steps, lambda: None)
                    emit({"leg": "launch", "what": what, "vocab": V, "B": B, "run": rnd, "us_per_launch": round(ms * 1e3 / chain, 2)})
            if B == 1:
                sampler_on_rows(chain, steps, V, dt, logits, con, list(kinds)[0], tok, rng, eos, emit)


def sampler_on_rows(chain, steps, V, dt, logits, con, sparse, tok, rng, eos, emit):
    """the fused top-k sampler (top_k 200) alone on the model's row and on the same row constrained to the sparse state's 64 tokens:
    fewer candidates than top_k put the pivot on -MAXF, which every banned entry ties with"""
    L, code = _lib.load(), runtime.dtype_code(dt)
    con.set_row(0, sparse)
    con.launch(logits, V, 1, tok, rng, eos.data_ptr())
    ws = runtime.new_workspace(64, V)
    state = torch.tensor([1234, 0], dtype=torch.int64, device="cuda")
    out, pos = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = torch.zeros(8, dtype=torch.int32, device="cuda")
    active = torch.ones(1, dtype=torch.int32, device="cuda")

    def make(row):
        def fn():
            st = runtime.stream_ptr()
            for _ in range(chain):
                _lib.check(L.teal_sample_topk_slot(row.data_ptr(), V, code, TOP_K, T, state.data_ptr(), out.data_ptr(), pos.data_ptr(),
                                                   hist.data_ptr(), 8, ws.data_ptr(), ws.numel() * 4, active.data_ptr(), 0, st),
                           "teal_sample_topk_slot")
        return fn

    graphs = [("teal_sample_topk_slot on the model's row", capture(make(logits[0]))),
              ("teal_sample_topk_slot on the row constrained to 64 tokens", capture(make(con.con[0])))]
    for rnd in (1, 2):
        for what, gr in graphs:
            ms = replay_ms(gr, steps, lambda: None)
            emit({"leg": "launch", "what": what, "vocab": V, "B": 1, "run": rnd, "us_per_launch": round(ms * 1e3 / chain, 2)})


def main():
    bench = FeatureBench("off,free,trie", note_eg="which build this is", library=_lib.LIB_OVERRIDE or "in-tree")
    a, legs = bench.a, bench.legs
    if "1" in legs or "2" in legs:
        m, ths, prompts = bench.model()
        for leg, B in (("1", 8), ("2", 1)):
            if leg in legs:
                leg_engine(bench, f"SlotDecodeEngine B={B}", m, ths, B, prompts)
    if "3" in legs:
        leg_launch(a.chain, a.steps, bench.dt, bench.emit)
    bench.close()


if __name__ == "__main__":
    main()
