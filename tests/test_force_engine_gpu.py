"""GPU: teacher-forced requests through SlotDecodeEngine and ContinuousBatcher on the synthetic `tiny-test` and `tiny-gqa-test`
models, fp16 and bf16, budgets <= 12, three slots for four requests (the fourth takes the slot of the first to finish).

Run A serves the four requests freely with seeds s_r and yields tokens D_r and logprobs L_r.  Then, per configuration:

  (a) exact replay: forced to D_r with other seeds and another temperature on the same admission schedule, every request's tokens,
      position, slot words, finish step and logprobs (with the top-1 alternate) are run A's, bit for bit — under TEAL thresholds
      and with every row kept: the same tokens are fed in the same slots on the same steps;
  (b) answer prefix: forced to D_r[:k] with seed s_r and the full budget, all tokens are D_r — the draw counter runs on;
  (c) a graph replay equals eager stepping, and sync_every 1 equals sync_every 8 (every row kept);
  (d) with every row kept a forced request leaves its unforced neighbours' tokens what they are without it;
  (e) the slot's next, unforced occupant draws freely and its length word is 0;
  (g) with every row kept "loglikelihood" is the sum over L_r and "is_greedy" agrees with "top_logprobs";
  (h) all of it also with kv_cache="fp8" and with per-request sampling on (the configurations below).

Once, on tiny-test: (f) a forced EOS id and a forced stop sequence end the request on that step and "forced" reports the shorter
count; the admission's refusals; and with the feature off a step and an admission launch what they launched before, on exactly one
launch more, between the samplers and the logprob launch.
"""
import functools
from collections import deque

import pytest
import torch

from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_BUDGET, SLOT_FINISH, SLOT_PRODUCED, SLOT_STEP, SlotDecodeEngine
from teal_amd.gpt_fast.constraints import Automaton
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_SEQ, B = 32, 3
T, TOP_K = 0.8, 50
PROMPTS = ([5, 9, 300, 9, 17], [44], [7, 7, 7, 450, 2, 2, 81, 6, 13, 250, 11], [1, 2, 3])
BUDGETS = (4, 12, 10, 9)      # request 0 ends first: request 3 takes its slot
SEEDS = (21, 22, 23, 24)
PREFIX_K = (2, 1, 5, 3)       # (b): how many of D_r are forced

CONFIGS = [("tiny-test", "fp16", "plain"), ("tiny-test", "bf16", "plain"), ("tiny-gqa-test", "fp16", "plain"),
           ("tiny-gqa-test", "bf16", "plain"), ("tiny-test", "fp16", "fp8"), ("tiny-gqa-test", "bf16", "fp8"),
           ("tiny-test", "fp16", "sampling"), ("tiny-gqa-test", "bf16", "sampling")]


@functools.lru_cache(maxsize=None)
def _model(name, precision, cache_batch):
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[precision]
    m = G.build_synthetic_model(name, DEV, dt, seed=3, std=0.05)
    ths = G.apply_sparsity(m, sparsity=0.5, hist_path=None, greedy_lookup=None, synthetic=True, decode_calibration=False)
    m.max_seq_length = -1
    m.setup_caches(max_batch_size=cache_batch, max_seq_length=MAX_SEQ)
    return m, ths


def _engine(name, precision, variant, dense):
    """a slot engine of B slots with logprobs (one alternate) on; dense: every row kept (thresholds -1)"""
    kv = "fp8" if variant == "fp8" else None
    m, ths = _model(name, precision, 1 if kv else B)
    if dense:
        ths = [{p: -1.0 for p in th} for th in ths]
    eng = SlotDecodeEngine(m, ths, B, kv_cache=kv)
    eng.set_logprobs(1)
    if variant == "sampling":
        eng.set_sampling_params(True)
    return eng


def _serve(eng, reqs, K=4, use_graph=True, temperature=T):
    """the batcher's loop on the bare engine: FIFO into free slots, K steps, harvest.  reqs: (prompt, budget, seed, admit keywords);
    -> per request what the engine left of it"""
    pending, slot_req, out = deque(range(len(reqs))), [None] * B, [None] * len(reqs)
    step0 = eng.read_state()[SLOT_STEP]
    while pending or any(r is not None for r in slot_req):
        for s in range(B):
            if slot_req[s] is None and pending:
                r = pending.popleft()
                prompt, budget, seed, kw = reqs[r]
                eng.admit(s, prompt, budget, None, seed, temperature, TOP_K, **kw)
                slot_req[s] = r
        eng.run_steps(K, temperature, TOP_K, use_graph)
        st = eng.read_state()
        for s in range(B):
            r = slot_req[s]
            if r is None or (st[SLOT_ACTIVE] >> s) & 1:
                continue
            n = st[SLOT_PRODUCED + s]
            lp, ids, tlp = eng.read_logprobs(s, n)
            out[r] = dict(tokens=eng.read_history(s, n), lp=lp, top_ids=ids, top_lp=tlp, slot=s, pos=int(eng.pos_buf[s]),
                          words=(st[SLOT_BUDGET + s], n), finish=st[SLOT_FINISH + s] - step0)
            slot_req[s] = None
    return out


def _reqs(variant, forced=None, seeds=SEEDS):
    extra = {"top_p": 0.9} if variant == "sampling" else {}
    return [(PROMPTS[r], BUDGETS[r], seeds[r], dict(extra, **({"forced_tokens": forced[r]} if forced and forced[r] else {})))
            for r in range(4)]


@pytest.mark.parametrize("name,precision,variant", CONFIGS)
def test_forced_requests_replay_the_free_run(name, precision, variant):
    other = tuple(s + 100 for s in SEEDS)
    for dense in (False, True):
        eng = _engine(name, precision, variant, dense)
        with pytest.raises(RuntimeError, match=r"forced tokens are off \(set_forced_tokens\)"):
            eng.admit(0, [1, 2], 3, None, 1, T, TOP_K, forced_tokens=[5])
        A = _serve(eng, _reqs(variant))
        D = [a["tokens"] for a in A]
        assert [len(d) for d in D] == list(BUDGETS) and A[3]["slot"] == A[0]["slot"] == 0
        key_off = eng._feature_key()
        eng.set_forced_tokens(True)
        key_on = eng._feature_key()
        assert eng._graph is None and key_on.count("forced") == 1 and tuple(k for k in key_on if k != "forced") == key_off
        # the feature on, nobody forced: run A again
        assert _serve(eng, _reqs(variant)) == A
        assert [eng.read_forced(s) for s in range(B)] == [0, 0, 0]
        # (a) exact replay, eager and captured (c)
        for use_graph in (True, False):
            got = _serve(eng, _reqs(variant, D, other), use_graph=use_graph, temperature=1.3)
            assert got == A, (dense, use_graph, [k for g, a in zip(got, A) for k in a if g[k] != a[k]])
        assert eng.read_forced(1) == BUDGETS[1] and eng.read_forced(0) == BUDGETS[3]
        # (b) answer prefix: the stream goes on where the counter stands
        got = _serve(eng, _reqs(variant, [d[:k] for d, k in zip(D, PREFIX_K)]))
        assert got == A, (dense, "prefix")
        if not dense:
            continue
        # (c) sync_every 1 and 8
        for K in (1, 8):
            got = _serve(eng, _reqs(variant, D, other), K=K, temperature=1.3)
            assert [g["tokens"] for g in got] == D and [(g["lp"], g["top_ids"], g["top_lp"]) for g in got] == \
                [(a["lp"], a["top_ids"], a["top_lp"]) for a in A], K
        # (d) a forced request among free neighbours, (e) and the free request that takes its slot
        W = [[3, 500, 3, 77], None, None, None]
        got = _serve(eng, _reqs(variant, W))
        assert got[0]["tokens"] == W[0] and got[0]["lp"] != A[0]["lp"]
        assert [g["tokens"] for g in got[1:]] == D[1:] and got[3]["slot"] == 0 and eng.read_forced(0) == 0
        assert got[1:] == A[1:]
        # (g) the batcher's sums are run A's
        V = eng.cfg.vocab_size
        rq = [Request(PROMPTS[r], BUDGETS[r], seed=other[r], forced_tokens=D[r], **({"top_p": 0.9} if variant == "sampling" else {}))
              for r in range(4)]
        res = ContinuousBatcher(eng, sync_every=4, temperature=1.3, top_k=TOP_K, logprobs=1).run(rq)
        assert res["tokens"] == D and res["forced"] == list(BUDGETS)
        for r in range(4):
            total = 0.0
            for v in A[r]["lp"]:
                total += float(v)
            assert res["loglikelihood"][r] == total and total < 0.0, r
            assert res["is_greedy"][r] == all(res["top_logprobs"][r][i][0][0] == D[r][i] for i in range(BUDGETS[r])), r
            assert all(0 <= res["top_logprobs"][r][i][0][0] < V for i in range(BUDGETS[r]))
        assert not all(res["is_greedy"])  # (36 draws at temperature 0.8 from 50 tokens: some were not the most likely one)
        # ... and a continuation made of top-1 tokens is greedy: forced to what top_k = 1 draws
        free = [Request(PROMPTS[r], BUDGETS[r]) for r in range(4)]
        greedy = ContinuousBatcher(eng, sync_every=4, temperature=T, top_k=1, logprobs=1).run(free)
        tops = [[t[0][0] for t in greedy["top_logprobs"][r]] for r in range(4)]
        rq = [Request(PROMPTS[r], BUDGETS[r], forced_tokens=greedy["tokens"][r]) for r in range(4)]
        res = ContinuousBatcher(eng, sync_every=4, temperature=T, top_k=TOP_K, logprobs=1).run(rq)
        assert res["is_greedy"] == [greedy["tokens"][r] == tops[r] for r in range(4)] and any(res["is_greedy"])
        assert res["logprobs"] == greedy["logprobs"] and res["tokens"] == greedy["tokens"]
        eng.set_forced_tokens(False)
        assert eng._feature_key() == key_off


@functools.lru_cache(maxsize=None)
def _tiny():
    return _engine("tiny-test", "fp16", "plain", True)


def test_a_forced_eos_and_a_forced_stop_sequence_end_the_request_on_that_step():
    eng = _tiny()
    eng.set_forced_tokens(True)
    E = 401
    # on the bare engine: the forced EOS is draw 2 — the admission's draw and two steps
    eng.admit(1, [5, 9, 300], 8, E, 31, T, TOP_K, forced_tokens=[17, 18, E, 19, 20])
    eng.run_steps(1, T, TOP_K)
    st = eng.read_state()
    assert (st[SLOT_ACTIVE] >> 1) & 1 and st[SLOT_PRODUCED + 1] == 2
    step = st[SLOT_STEP]
    eng.run_steps(1, T, TOP_K)
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0 and st[SLOT_PRODUCED + 1] == 3 and st[SLOT_FINISH + 1] == step
    assert eng.read_history(1, 3) == [17, 18, E]
    # a forced first token that is the EOS id ends the request at its admission
    eng.admit(2, [5, 9], 8, E, 31, T, TOP_K, forced_tokens=[E, 19])
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0 and st[SLOT_PRODUCED + 2] == 1 and eng.read_history(2, 1) == [E]
    # through the batcher, next to a stop sequence and a free request
    reqs = [Request([5, 9, 300], 8, E, forced_tokens=[17, 18, E, 19, 20]),
            Request([8, 3], 8, stop_sequences=[[61, 62]], forced_tokens=[60, 61, 62, 63, 64]),
            Request([1, 2, 3], 6),
            Request([4, 4], 8, stop_token_ids=[70], min_new_tokens=3, forced_tokens=[70, 71, 70, 72])]  # held back at draw 0
    out = {}
    for K in (1, 8):
        res = ContinuousBatcher(eng, sync_every=K, temperature=T, top_k=TOP_K, finish_reason=True).run(reqs)
        assert res["tokens"][0] == [17, 18, E] and res["tokens"][1] == [60, 61, 62] and res["tokens"][3] == [70, 71, 70]
        assert len(res["tokens"][2]) == 6
        assert res["forced"] == [3, 3, None, 3] and res["finish_reason"] == ["stop_token", "stop_sequence", "length", "stop_token"]
        assert res["stop_match"] == [E, 0, -1, 70]
        assert [len(x) for x in res["logprobs"]] == [3, 3, 6, 3] and res["is_greedy"][2] is None
        for r in (0, 1, 3):
            total = 0.0
            for v in res["logprobs"][r]:
                total += v
            assert res["loglikelihood"][r] == total
        out[K] = {k: res[k] for k in ("tokens", "forced", "loglikelihood", "is_greedy", "logprobs")}
    assert out[1] == out[8]
    eng.set_stop_conditions(False)
    eng.set_logprobs(1)
    eng.set_forced_tokens(False)


def test_the_admissions_refusals_leave_the_slot_as_it_was():
    eng = _tiny()
    eng.set_forced_tokens(True, capacity=4)
    assert eng._forced().table.shape == (8, 4) and eng._forced().lengths.tolist() == [0] * 8
    eng.admit(0, [1, 2], 5, None, 1, T, TOP_K, forced_tokens=[9, 8])
    eng.run_steps(5, T, TOP_K)
    before = (eng.read_state(), eng.read_forced(0), eng._forced().table.clone(), eng.tok_buf.clone(), eng.pos_buf.clone())
    V = eng.cfg.vocab_size
    for kw, exc, why in ((dict(forced_tokens=[V]), ValueError, f"forced token id {V} is outside the vocabulary"),
                         (dict(forced_tokens=[-1]), ValueError, "outside the vocabulary"),
                         (dict(forced_tokens=[1, 2, 3, 4, 5]), ValueError, "5 forced tokens: the table holds 4"),
                         (dict(forced_tokens=[1, 2, 3, 4], budget=3), ValueError, "4 forced tokens exceed the request's budget of 3")):
        budget = kw.pop("budget", 8)
        with pytest.raises(exc, match=why):
            eng.admit(0, [1, 2], budget, None, 1, T, TOP_K, **kw)
    eng.set_constraints(True)
    eng.register_constraint("yn", Automaton.from_allowed([1, 2]))
    with pytest.raises(ValueError, match="forced tokens do not combine with a constraint"):
        eng.admit(0, [1, 2], 8, None, 1, T, TOP_K, constraint="yn", forced_tokens=[1])
    eng.set_constraints(False)
    after = (eng.read_state(), eng.read_forced(0), eng._forced().table, eng.tok_buf, eng.pos_buf)
    assert after[:2] == before[:2] and all(torch.equal(a, b) for a, b in zip(after[2:], before[2:]))
    with pytest.raises(ValueError, match="slot 3 outside"):
        eng.read_forced(3)
    eng.admit(0, [1, 2], 5, None, 1, T, TOP_K)  # the next occupant: its length word is written, to 0
    assert eng.read_forced(0) == 0
    with pytest.raises(RuntimeError, match="set_forced_tokens needs an idle engine"):
        eng.set_forced_tokens(False)
    eng.run_steps(5, T, TOP_K)
    eng.set_forced_tokens(False)
    with pytest.raises(RuntimeError, match="forced tokens are off"):
        eng.read_forced(0)
    eng.set_forced_tokens(True)  # the default capacity: a row per cache row
    assert eng._forced().table.shape == (8, MAX_SEQ)
    eng.set_forced_tokens(False)


class _Count:
    """a library handle that records which entry points are called"""

    def __init__(self, L, calls):
        self._L, self._calls = L, calls

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("teal_"):
            return f

        def call(*a):
            self._calls.append(name)
            return f(*a)
        return call


def test_off_the_launches_are_the_old_ones_and_on_there_is_one_more():
    eng = _tiny()
    eng.set_forced_tokens(False)
    eng.set_stop_conditions(False)
    eng.set_logprobs(1)

    def calls_of(what):
        calls = []
        holders = [eng, eng._lp] + ([eng._frc] if eng._frc is not None else [])
        keep = [h.L for h in holders]
        for h in holders:
            h.L = _Count(h.L, calls)
        try:
            what()
        finally:
            for h, L in zip(holders, keep):
                h.L = L
        return calls

    def admit_all():
        for s in range(B):
            eng.admit(s, PROMPTS[s], 6, None, SEEDS[s], T, TOP_K)

    step = lambda: eng._self_step(T, TOP_K)  # noqa: E731
    admit = lambda: eng.admit(0, [1, 2, 3], 2, None, 5, T, TOP_K)  # noqa: E731
    admit_all()
    off = calls_of(step)
    n_layers = len(eng.model.layers)
    # embedding rows; per layer qkv, attention, wo, resid, gate|up, down, resid; lm_head and its rounding; B samplers; logprobs; retire
    assert len(off) == 1 + 7 * n_layers + 2 + B + 2 and off[-2:] == ["teal_token_logprobs", "teal_batched_retire"]
    assert "teal_force_tokens" not in off
    eng.run_steps(6, T, TOP_K, use_graph=False)
    admit_off = calls_of(admit)
    assert admit_off[-3:] == ["teal_sample_topk_slot", "teal_token_logprobs", "teal_batched_retire"] and "teal_force_tokens" not in admit_off
    eng.run_steps(2, T, TOP_K, use_graph=False)
    eng.set_forced_tokens(True)
    admit_all()
    on = calls_of(step)
    assert on == off[:-2] + ["teal_force_tokens"] + off[-2:] and on[-4] == "teal_sample_topk_slot"
    eng.run_steps(6, T, TOP_K, use_graph=False)
    admit_on = calls_of(admit)
    assert admit_on == admit_off[:-2] + ["teal_force_tokens"] + admit_off[-2:]
    eng.run_steps(2, T, TOP_K, use_graph=False)
    eng.set_forced_tokens(False)
    admit_all()
    assert calls_of(step) == off
    eng.run_steps(6, T, TOP_K, use_graph=False)
    assert calls_of(admit) == admit_off
    eng.run_steps(2, T, TOP_K, use_graph=False)


def test_generate_requests_and_score_batched_end_to_end(tmp_path):
    import json
    import math
    from teal_amd.gpt_fast import score as S
    f = tmp_path / "reqs.jsonl"
    f.write_text('{"tokens": [1, 2, 3], "forced_tokens": [7, 8, 9, 10]}\n'
                 '{"tokens": [4], "max_new_tokens": 6, "seed": 5}\n'
                 '{"tokens": [5, 6, 7, 8, 9], "max_new_tokens": 7, "forced_tokens": [11, 12]}\n')
    res = G.main(G.build_parser().parse_args(["--device", "cuda", "--synthetic", "tiny-test", "--sparsity", "0.5", "--num_samples", "1",
                                              "--max_new_tokens", "12", "--compile", "--requests", str(f), "--batch_size", "2"]))
    seqs = res["sequences"]
    assert [len(s) for s in seqs] == [4, 6, 7] and seqs[0] == [7, 8, 9, 10] and seqs[2][:2] == [11, 12]
    assert res["forced"] == [4, None, 2] and res["is_greedy"][1] is None and res["loglikelihood"][1] is None
    for r in (0, 2):
        total = 0.0
        for v in res["logprobs"][r][:res["forced"][r]]:
            total += v
        assert res["loglikelihood"][r] == total < 0.0
    with pytest.raises(SystemExit, match="request 0: forced token id 512 is outside the vocabulary"):
        f.write_text('{"tokens": [1], "forced_tokens": [512]}\n')
        G.main(G.build_parser().parse_args(["--device", "cuda", "--synthetic", "tiny-test", "--sparsity", "0.5", "--num_samples", "1",
                                            "--compile", "--requests", str(f), "--batch_size", "2"]))
    # score.py: the same windows one at a time and three per batched step
    t = tmp_path / "tokens.jsonl"
    g = torch.Generator().manual_seed(9)
    t.write_text("\n".join(json.dumps({"tokens": torch.randint(0, 512, (n,), generator=g).tolist()}) for n in (30, 12, 17, 1)) + "\n")
    base = ["--synthetic", "tiny-test", "--sparsity", "0.5", "--tokens", str(t), "--window", "12"]
    one = S.main(S.build_parser().parse_args(base))
    many = S.main(S.build_parser().parse_args(base + ["--batch_size", "3"]))
    assert many["batch_size"] == 3 and "batch_size" not in one
    assert (many["windows"], many["scored_tokens"], many["window"]) == (one["windows"], one["scored_tokens"], one["window"]) == (6, 53, 12)
    assert all(math.isfinite(many[k]) and many[k] > 1.0 for k in ("perplexity", "perplexity_dense"))
    # every row kept, the two paths differ by the rounding of differently grouped sums into 16-bit logits (2^-11 relative per
    # logit, a few 1e-3 in a logprob): 1e-2 in the perplexity is ten times that.  At the sparsity nothing is asserted: a hard
    # threshold turns a rounding difference into a kept or dropped row
    assert abs(many["perplexity_dense"] / one["perplexity_dense"] - 1.0) < 1e-2
    for bad in ("1", "9"):
        with pytest.raises(SystemExit, match="--batch_size must be in 2..8"):
            S.main(S.build_parser().parse_args(base + ["--batch_size", bad]))
