"""GPU: per-request stop conditions through SlotDecodeEngine, ContinuousBatcher and generate.py on `tiny-test` with every row kept
(a request's tokens then do not depend on its neighbours: tests/test_logit_engine_gpu.py says why), MAX_SEQ = 64.  Three requests
run with the feature off first; their streams R_r are the reference every test shares.  The truth is the host model
(tests/stop_rule.py) run over R_r: with the feature on a request's tokens are R_r cut where the model fires.

  1. a stop id, a 3-token stop sequence and a min_new_tokens chosen from R_r — an id equal to R_r[0] (the request ends at admission)
     and an id that appears below min_new_tokens and again above it among them: tokens, reason and match are the model's, stepped
     eagerly and from the captured step;
  2. a request without stop conditions next to requests with them draws exactly R_r;
  3. through ContinuousBatcher with more requests than slots: tokens, finish_reason and stop_match are the model's for sync_every 1
     and 8, and a slot's next occupant does not inherit its row;
  4. on a registered prefix a stop sequence equal to the prompt's last tokens does not fire;
  5. next to logit processors, per-request sampling and logprobs the stop lands on the model's token and the logprob list is as
     long as the tokens;
  6. generate.py --requests end to end on a file mixing the new fields;
  7. with the feature off a step and an admission launch what they launched before; on, one launch takes the retire launch's place.
"""
import functools

import pytest
import torch

import stop_rule as R
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_PRODUCED, SlotDecodeEngine
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from test_logit_engine_gpu import _calls_of, _Count, _main, _model

pytestmark = pytest.mark.gpu
MAX_SEQ, BUDGET = 64, 24
KW = dict(temperature=0.8, top_k=3)  # a narrow filter: 24 draws repeat a token, which the min_new_tokens case needs

# slot: (prompt, budget, seed)
REQS3 = {0: ([5, 9, 300, 9, 17], BUDGET, 21), 1: ([44], BUDGET - 2, 22), 2: ([7, 7, 7, 450, 2, 2, 81, 6, 13, 250, 11], BUDGET, 23)}


@functools.lru_cache(maxsize=None)
def _engine():
    m, ths = _model("tiny-test", None, 3, max_seq=MAX_SEQ, sparsity=0.0)
    return SlotDecodeEngine(m, ths, 3)


def _run(eng, reqs, stops=None, use_graph=True, steps=BUDGET):
    """admit `reqs` (slot -> (prompt, budget, seed)) with `stops` (slot -> admit keywords) and run: slot -> tokens"""
    for s, (prompt, budget, seed) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **KW, **(stops or {}).get(s, {}))
    eng.run_steps(steps, use_graph=use_graph, **KW)
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0
    return {s: eng.read_history(s, st[SLOT_PRODUCED + s]) for s in reqs}


@functools.lru_cache(maxsize=None)
def _streams():
    """R_r: what the three requests draw with the feature off"""
    eng = _engine()
    eng.set_stop_conditions(False)
    got = _run(eng, REQS3)
    assert [len(got[s]) for s in REQS3] == [REQS3[s][1] for s in REQS3]
    return got


def _want(stream, budget, **kw):
    return R.fire(stream, budget, **kw)


def _repeat(stream):
    """(token, i, j): a token drawn at i and again at j > i + 1, the earliest such j — or None"""
    best = None
    for j, t in enumerate(stream):
        first = stream.index(t)
        if j > first + 1 and (best is None or j < best[2]):
            best = (t, first, j)
    return best


def _chosen():
    """slot -> admit keywords chosen from R_r: an id equal to R_r[0]; an id below and again above min_new_tokens; a 3-token sequence
    next to one that never matches and a one-token sequence of a higher index"""
    Rr = _streams()
    rep = {s: _repeat(Rr[s]) for s in Rr}
    held = next((s for s in Rr if rep[s] is not None), None)
    assert held is not None, ("no request repeats a token: choose other seeds", Rr)
    first, seq = [s for s in Rr if s != held]
    t, i, j = rep[held]
    k = 11
    return {first: dict(stop_token_ids=[1000 % 512, Rr[first][0]]),
            held: dict(stop_token_ids=[t], min_new_tokens=i + 2),  # at draw i only i + 1 tokens are produced: held back; at j it fires
            seq: dict(stop_sequences=[[3, 4, 5], Rr[seq][k - 2:k + 1], Rr[seq][k:k + 1]], min_new_tokens=2)}, held


def test_tokens_reason_and_match_are_the_models_eager_and_captured():
    Rr = _streams()
    stops, held = _chosen()
    eng = _engine()
    with pytest.raises(RuntimeError, match=r"stop conditions are off \(set_stop_conditions\)"):
        eng.admit(0, [1, 2], 3, None, 1, **KW, stop_token_ids=[5])
    with pytest.raises(RuntimeError, match="off"):
        eng.read_finish(0)
    eng.admit(0, [1, 2], 1, None, 1, **KW, stop_token_ids=(), stop_sequences=(), min_new_tokens=0)  # spelled-out "none" needs nothing
    eng.set_stop_conditions(True)
    want = {s: _want(Rr[s], REQS3[s][1], **stops[s]) for s in REQS3}
    kinds = {w[1] for w in want.values()}
    assert kinds == {"stop_token", "stop_sequence"}, want
    assert min(len(w[0]) for w in want.values()) == 1 and len(want[held][0]) > stops[held]["min_new_tokens"] - 1
    for use_graph in (False, True):
        got = _run(eng, REQS3, stops, use_graph=use_graph)
        for s in REQS3:
            assert (got[s],) + eng.read_finish(s) == want[s], (use_graph, s)
    g = eng._graph
    assert g is not None
    _run(eng, REQS3, {s: stops[(s + 1) % 3] for s in REQS3})  # other rows in the same slots: the same captured step
    assert eng._graph is g
    for bad, msg in [(dict(stop_token_ids=[512]), "outside the vocabulary"), (dict(stop_sequences=[[]]), "empty"),
                     (dict(stop_sequences=[[1] * 9]), "at most 8"), (dict(min_new_tokens=-1), "non-negative")]:
        with pytest.raises(ValueError, match=msg):
            eng.admit(0, [1, 2], 3, None, 1, **KW, **bad)
    assert eng.read_state()[SLOT_ACTIVE] == 0  # refused before anything moved
    eng.admit(0, [1, 2], 5, None, 1, **KW)
    with pytest.raises(RuntimeError, match="idle"):
        eng.set_stop_conditions(False)
    eng.run_steps(5, **KW)
    assert eng.read_finish(0) == ("length", -1)


def test_a_request_without_stop_conditions_draws_what_it_drew():
    Rr = _streams()
    stops, held = _chosen()
    eng = _engine()
    eng.set_stop_conditions(True)
    for plain in REQS3:
        got = _run(eng, REQS3, {s: kw for s, kw in stops.items() if s != plain})
        assert got[plain] == Rr[plain] and eng.read_finish(plain) == ("length", -1), plain
        # ... also in a slot whose last occupant left a row that would have stopped it
        moved = {(plain + 1) % 3: REQS3[plain]}
        _run(eng, moved, {(plain + 1) % 3: dict(stop_token_ids=Rr[plain][:4])})
        assert _run(eng, moved)[(plain + 1) % 3] == Rr[plain]
    eng.set_stop_conditions(False)
    assert _run(eng, REQS3) == Rr and eng.stop_table is None


def test_through_the_batcher_slots_are_reused_and_rows_are_not_inherited():
    eng = _engine()
    eng.set_stop_conditions(False)
    prompts = [[5, 9, 300, 9, 17], [44], [7, 7, 7, 450, 2, 2], [1, 2, 3], [100, 200], [8], [9, 9, 9, 9]]
    budgets = [20, 9, 20, 16, 20, 12, 20]
    plain = [Request(p, n) for p, n in zip(prompts, budgets)]
    base = ContinuousBatcher(eng, sync_every=4, **KW).run(plain)
    full = base["tokens"]
    assert "finish_reason" not in base and eng.stop_table is None and [len(t) for t in full] == budgets
    later = [full[r][1] for r in (3, 4, 5, 6)]  # ids that would stop the later requests at once, had they inherited a row
    specs = [dict(stop_token_ids=later + [full[0][6]]), dict(stop_token_ids=later, stop_sequences=[full[1][2:5]]),
             dict(stop_token_ids=later + [full[2][0]]), dict(), dict(stop_sequences=[full[4][7:8]], min_new_tokens=3), dict(),
             dict(stop_token_ids=[full[6][2]], min_new_tokens=8)]
    reqs = [Request(p, n, **kw) for p, n, kw in zip(prompts, budgets, specs)]
    want = [_want(full[r], budgets[r], **specs[r]) for r in range(len(reqs))]
    assert want[3] == (full[3], "length", -1) and want[5] == (full[5], "length", -1) and len(want[2][0]) == 1
    out = {}
    for K in (1, 8):
        res = ContinuousBatcher(eng, sync_every=K, **KW).run(reqs)
        assert eng.stop_table is not None
        got = list(zip(res["tokens"], res["finish_reason"], res["stop_match"]))
        assert got == want, K
        assert len(set(res["slots"])) == 3 and res["admissions"] == 7
        out[K] = got
    assert out[1] == out[8]
    eng.set_stop_conditions(False)


def test_a_stop_sequence_equal_to_the_prompts_last_tokens_does_not_fire():
    eng = _engine()
    eng.set_stop_conditions(False)
    pre, suffix, budget = [400, 401, 402, 9, 400, 77, 78, 79, 80], [5, 9, 300], 12
    if not eng.has_prefix("sys"):
        eng.register_prefix("sys", pre)

    def run(**kw):
        eng.admit(1, suffix, budget, None, 41, **KW, prefix="sys", **kw)
        eng.run_steps(budget, **KW)
        st = eng.read_state()
        assert st[SLOT_ACTIVE] == 0
        return eng.read_history(1, st[SLOT_PRODUCED + 1])

    full = run()
    assert len(full) == budget
    eng.set_stop_conditions(True)
    # the prefix's last tokens, the suffix's, and the prompt's tail running into the first generated tokens: none is a match, for a
    # sequence is compared with generated tokens only
    kw = dict(stop_sequences=[pre[-3:], suffix[-3:], pre[-1:] + suffix, suffix[-2:] + full[:1], suffix[-1:] + full[:2], pre[-1:]])
    want = _want(full, budget, **kw)
    got = run(**kw)
    assert (got,) + eng.read_finish(1) == want
    if not set(pre[-1:]) & set(full):
        assert want == (full, "length", -1)
    kw = dict(stop_sequences=[suffix[-1:] + full[:2], full[:2]])  # ... and the generated part of it alone is
    got = run(**kw)
    assert (got,) + eng.read_finish(1) == (full[:2], "stop_sequence", 1) == _want(full, budget, **kw)
    eng.set_stop_conditions(False)


def test_next_to_processors_sampling_and_logprobs_the_stop_lands_on_the_models_token():
    m, ths = _model("tiny-test", None, 2, max_seq=MAX_SEQ, sparsity=0.0)
    eng = SlotDecodeEngine(m, ths, 2)
    reqs = [Request([5, 9, 300, 9], 16, repetition_penalty=1.3, top_p=0.9), Request([8, 3], 16, frequency_penalty=0.7, min_p=0.02),
            Request([1, 2, 3], 10, logit_bias={"77": 3.0})]
    kw = dict(sync_every=3, logprobs=1, temperature=0.8, top_k=20)
    base = ContinuousBatcher(eng, **kw).run(reqs)
    full = base["tokens"]
    assert "finish_reason" not in base and [len(t) for t in full] == [16, 16, 10]
    specs = [dict(stop_token_ids=[full[0][5]]), dict(stop_sequences=[full[1][6:9]], min_new_tokens=4), dict()]
    on = [Request(q.tokens, q.max_new_tokens, repetition_penalty=q.repetition_penalty, frequency_penalty=q.frequency_penalty,
                  logit_bias=q.logit_bias, top_p=q.top_p, min_p=q.min_p, **s) for q, s in zip(reqs, specs)]
    res = ContinuousBatcher(eng, **kw).run(on)
    want = [_want(full[r], reqs[r].max_new_tokens, **specs[r]) for r in range(3)]
    assert list(zip(res["tokens"], res["finish_reason"], res["stop_match"])) == want
    assert len(want[0][0]) <= 6 and want[1][1] == "stop_sequence" and want[2][1] == "length"
    for r in range(3):
        n = len(res["tokens"][r])
        assert len(res["logprobs"][r]) == n == len(res["top_logprobs"][r])
        assert res["logprobs"][r] == base["logprobs"][r][:n]  # the same draws from the same rows, up to the stop


def test_generate_requests_end_to_end_with_stop_fields(tmp_path):
    f = tmp_path / "reqs.jsonl"
    lines = ['{"tokens": [1, 2, 3], "seed": 3}', '{"tokens": [4], "max_new_tokens": 20, "seed": 5}',
             '{"tokens": [5, 6, 7, 8, 9], "max_new_tokens": 14, "seed": 7}', '{"tokens": [10, 11], "max_new_tokens": 20, "seed": 8}',
             '{"tokens": [10, 12], "max_new_tokens": 6, "seed": 9}']
    f.write_text("\n".join(lines) + "\n")
    args = ("--compile", "--requests", str(f), "--batch_size", "2", "--sparsity", "0.0")
    base = _main(*args)
    full = base["sequences"]
    assert [len(s) for s in full] == [12, 20, 14, 20, 6] and "finish_reason" not in base
    flag_id = full[4][3]
    specs = [dict(stop_token_ids=[full[0][4]]), dict(stop_sequences=[full[1][7:10]], min_new_tokens=5), dict(stop_token_ids=[]),
             dict(stop_token_ids=[full[3][0]], min_new_tokens=3), dict()]
    import json
    f.write_text("\n".join(json.dumps({**json.loads(ln), **s}) for ln, s in zip(lines, specs)) + "\n")
    res = _main(*args, "--stop_token_ids", str(flag_id), "--min_new_tokens", "2")
    budgets = [12, 20, 14, 20, 6]
    for r, s in enumerate(specs):
        kw = {"stop_token_ids": [flag_id], "min_new_tokens": 2, **s}  # the flags are the defaults of requests that set none
        assert (res["sequences"][r], res["finish_reason"][r], res["stop_match"][r]) == _want(full[r], budgets[r], **kw), r
    assert res["finish_reason"][4] == "stop_token" and res["stop_match"][4] == flag_id and res["finish_reason"][2] == "length"
    only = _main(*args, "--finish_reason")
    assert only["sequences"][:2] != full[:2] and only["finish_reason"][2] == "length" and only["sequences"][2] == full[2]
    with pytest.raises(SystemExit, match="request 1: stop token id 512"):
        f.write_text('{"tokens": [1]}\n{"tokens": [1], "stop_token_ids": [512]}\n')
        _main(*args)


def test_with_the_feature_off_a_step_and_an_admission_launch_what_they_launched():
    B = 3
    m, ths = _model("tiny-test", None, B, max_seq=MAX_SEQ)
    eng = SlotDecodeEngine(m, ths, B)

    def calls_of(step):
        if eng._stops is not None:
            keep, calls = eng._stops.L, []
            eng._stops.L = _Count(keep, calls)
            try:
                return _calls_of(eng, step) + calls
            finally:
                eng._stops.L = keep
        return _calls_of(eng, step)

    def admit_all():
        for s, (p, b, seed) in REQS3.items():
            eng.admit(s, p, b, None, seed, **KW)

    step = lambda: eng._self_step(**KW)  # noqa: E731
    admit = lambda: eng.admit(0, [1, 2, 3], 2, None, 5, **KW)  # noqa: E731
    admit_all()
    fresh = calls_of(step)
    n_layers = len(m.layers)
    # embedding rows; per layer qkv, attention, wo, resid, gate|up, down, resid; lm_head and its rounding; B samplers; retire
    assert len(fresh) == 1 + 7 * n_layers + 2 + B + 1 and fresh[-1] == "teal_batched_retire" and "teal_batched_retire_stops" not in fresh
    eng.run_steps(BUDGET, use_graph=False, **KW)
    admit_fresh = calls_of(admit)
    assert admit_fresh[-1] == "teal_batched_retire" and "teal_batched_retire_stops" not in admit_fresh
    eng.run_steps(2, use_graph=False, **KW)
    eng.set_stop_conditions(True)
    admit_all()
    on = calls_of(step)
    assert len(on) == len(fresh) and on[:-1] == fresh[:-1] and on[-1] == "teal_batched_retire_stops"
    assert "teal_batched_retire" not in on
    eng.run_steps(BUDGET, use_graph=False, **KW)
    admit_on = calls_of(admit)
    assert len(admit_on) == len(admit_fresh) and admit_on[-1] == "teal_batched_retire_stops" and "teal_batched_retire" not in admit_on
    eng.run_steps(2, use_graph=False, **KW)
    assert eng.stop_table.shape == (8, 96) and eng.stop_table.dtype == torch.int32
    eng.set_stop_conditions(False)
    admit_all()
    assert calls_of(step) == fresh and eng.stop_table is None
    eng.run_steps(BUDGET, use_graph=False, **KW)
    assert calls_of(admit) == admit_fresh
