"""GPU: constrained decoding through SlotDecodeEngine, ContinuousBatcher and generate.py on `tiny-test` (vocab 512) with every row
kept, B = 3, MAX_SEQ = 64 (a request's tokens then do not depend on its neighbours: tests/test_logit_engine_gpu.py says why).

  1. a `choices` request yields exactly one choice followed by its EOS id and ends on that step for sync_every 1 and 8; its trace
     is the trie path and carries no violation bit;
  2. unconstrained neighbours draw bit for bit what they draw with the feature off; a slot re-admitted without a constraint after
     a constrained request is unconstrained; changing constraints between admissions keeps the captured step;
  3. with logit processors and per-request sampling on the chain is adjust -> constrain -> sample (a bias cannot open a banned
     token); with min_new_tokens an accepting state below the minimum draws an EOS id that is ignored and leaves the state in place;
  4. `allowed_token_ids` at temperature 1.5: 200 drawn tokens all lie in the set;
  5. the refusals; generate.py --requests with --constraints and "choices" lines end to end;
  6. with the feature off a step and an admission launch what they launched before; on, one launch more, in front of the samplers.
"""
import functools
import json

import pytest

from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_PRODUCED, BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.constraints import VIOLATION, Automaton
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from teal_amd.gpt_fast.engine import DecodeEngine
from test_logit_engine_gpu import _Count, _main, _model

pytestmark = pytest.mark.gpu
MAX_SEQ, BUDGET, EOS = 64, 16, 500
KW = dict(temperature=0.8, top_k=50)
CHOICES = [[11], [11, 12], [20, 21, 22], [20, 30, 31, 32], [40, 41]]  # 1..4 tokens; shared prefixes; one a prefix of another
ALLOWED = [3, 17, 64, 65, 130, 255, 256, 300, 411, 511]

# slot: (prompt, budget, seed)
REQS3 = {0: ([5, 9, 300, 9, 17], BUDGET, 21), 1: ([44], BUDGET - 2, 22), 2: ([7, 7, 7, 450, 2, 2, 81, 6, 13, 250, 11], BUDGET, 23)}


@functools.lru_cache(maxsize=None)
def _engine():
    m, ths = _model("tiny-test", None, 3, max_seq=MAX_SEQ, sparsity=0.0)
    return SlotDecodeEngine(m, ths, 3)


def _fresh(on=True):
    """the shared engine, idle, with the feature switched (a switch drops every registered constraint)"""
    eng = _engine()
    assert eng.read_state()[SLOT_ACTIVE] == 0
    eng.set_stop_conditions(False)
    eng.set_sampling_params(False)
    eng.set_constraints(on)
    return eng


def _run(eng, reqs, extra=None, use_graph=True, steps=BUDGET, eos=None):
    """admit `reqs` (slot -> (prompt, budget, seed)) with `extra` (slot -> admit keywords) and run: slot -> tokens"""
    for s, (prompt, budget, seed) in reqs.items():
        kw = dict((extra or {}).get(s, {}))
        eng.admit(s, prompt, budget, kw.pop("eos_id", eos), seed, **KW, **kw)
    eng.run_steps(steps, use_graph=use_graph, **KW)
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0
    return {s: eng.read_history(s, st[SLOT_PRODUCED + s]) for s in reqs}


@functools.lru_cache(maxsize=None)
def _streams():
    """what the three requests draw with the feature off: the reference the tests share"""
    got = _run(_fresh(False), REQS3)
    assert [len(got[s]) for s in REQS3] == [REQS3[s][1] for s in REQS3]
    return got


def _path(a, tokens, eos):
    """the states the draws of `tokens` were made in: the automaton walked on the host"""
    s, out = 0, []
    for t in tokens:
        out.append(s)
        if t != eos:
            s = a.delta(s, t)
            assert s >= 0
    return out


def test_a_choices_request_yields_one_choice_then_eos_and_its_trace_is_the_trie_path():
    eng = _fresh()
    a = Automaton.from_choices(CHOICES)
    eng.register_constraint("pick", a)
    seen = set()
    for use_graph in (False, True):
        for seed in (1, 2, 3, 4, 5, 6):
            reqs = {s: ([5 + s, 9, 30 + seed], BUDGET, 10 * seed + s) for s in range(3)}
            got = _run(eng, reqs, {s: dict(constraint="pick", eos_id=EOS) for s in reqs}, use_graph=use_graph)
            for s, toks in got.items():
                assert toks[-1] == EOS and toks[:-1] in CHOICES, toks          # one choice, then the EOS id: it ended on that step
                trace = eng.read_constraint_trace(s, len(toks))
                assert trace == _path(a, toks, EOS) and not any(w & VIOLATION for w in trace)
                seen.add(tuple(toks[:-1]))
    assert len(seen) >= 2, seen  # (the model chooses: not one choice over and over)
    # through the batcher, more requests than slots: the same for sync_every 1 and 8
    reqs = [Request([5 + r, 9, 300], BUDGET, eos_id=EOS, choices=CHOICES if r % 3 else CHOICES[::-1]) for r in range(7)]
    out = {}
    for K in (1, 8):
        res = ContinuousBatcher(eng, sync_every=K, **KW).run(reqs)
        for toks in res["tokens"]:
            assert toks[-1] == EOS and toks[:-1] in CHOICES, (K, toks)
        out[K] = res["tokens"]
    assert out[1] == out[8]
    assert sum(n.startswith("choices:") for n in eng._con.images) == 1  # one image for the seven requests: keyed by content


def test_unconstrained_neighbours_and_readmission_draw_what_they_drew_and_the_graph_stays():
    Rr = _streams()
    eng = _fresh()
    eng.register_constraint("set", Automaton.from_allowed(ALLOWED))
    eng.register_constraint("pick", Automaton.from_choices(CHOICES))
    for con in REQS3:
        got = _run(eng, REQS3, {con: dict(constraint="set")})
        assert all(t in ALLOWED for t in got[con]) and len(got[con]) == REQS3[con][1]
        assert all(got[s] == Rr[s] for s in REQS3 if s != con), con  # the neighbours: bit for bit the feature-off tokens
        assert eng.read_constraint_trace((con + 1) % 3, 4) == [0, 0, 0, 0]
        # the slot's next occupant does not inherit the constraint
        moved = {con: REQS3[con]}
        assert _run(eng, moved)[con] == Rr[con]
    g = eng._graph
    assert g is not None
    _run(eng, REQS3, {0: dict(constraint="pick", eos_id=EOS), 2: dict(constraint="set")})  # other automata in other slots ...
    assert eng._graph is g                                                                 # ... the same captured step
    assert _run(eng, REQS3) == Rr
    eng.set_constraints(False)
    assert eng._graph is None and _run(eng, REQS3) == Rr


def _calls(eng, step):
    """the entry points `step` calls through every library handle of the engine"""
    calls, keep = [], eng.L
    holders = [eng] + [f for f in (eng._proc, eng._samp, eng._con, eng._stops, eng._lp) if f is not None]
    for h in holders:
        h.L = _Count(keep, calls)
    try:
        step()
    finally:
        for h in holders:
            h.L = keep
    return calls


def test_with_processors_and_sampling_the_chain_is_adjust_constrain_sample():
    m, ths = _model("tiny-test", None, 2, max_seq=MAX_SEQ, sparsity=0.0)
    eng = SlotDecodeEngine(m, ths, 2)
    for on in (eng.set_logit_processors, eng.set_sampling_params, eng.set_constraints):
        on(True)
    eng.register_constraint("set", Automaton.from_allowed(ALLOWED))
    # a bias far above every logit on a banned token and on an allowed one: the constraint is applied behind the bias
    eng.admit(0, [5, 9, 300], 12, None, 7, temperature=0.8, top_k=50, top_p=0.9, logit_bias={7: 200.0, 64: 150.0}, constraint="set")
    eng.admit(1, [8, 3], 12, None, 8, temperature=0.8, top_k=50, min_p=0.02, logit_bias={7: 200.0})
    calls = _calls(eng, lambda: eng._self_step(0.8, 50))
    tail = calls[calls.index("teal_logit_adjust"):]
    assert tail == ["teal_logit_adjust", "teal_constrain_logits", "teal_sample_rows", "teal_batched_retire"], tail
    eng.run_steps(12)
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0
    assert eng.read_history(0, st[SLOT_PRODUCED]) == [64] * 12       # the biased allowed token; the banned one never
    assert eng.read_history(1, st[SLOT_PRODUCED + 1]) == [7] * 12    # the unconstrained neighbour follows its bias
    admit = _calls(eng, lambda: eng.admit(0, [1, 2, 3], 1, None, 5, temperature=0.8, top_k=50, constraint="set"))
    assert admit[-4:] == ["teal_logit_adjust", "teal_constrain_logits", "teal_sample_rows", "teal_batched_retire"], admit


def test_below_min_new_tokens_an_accepting_state_draws_an_eos_that_is_ignored():
    eng = _fresh()
    eng.set_stop_conditions(True)
    a = Automaton.from_choices([[40, 41]])
    eng.register_constraint("one", a)
    for use_graph in (False, True):
        got = _run(eng, {1: ([5, 9], BUDGET, 3)}, {1: dict(constraint="one", eos_id=EOS, min_new_tokens=5)}, use_graph=use_graph)
        # after 40, 41 only the EOS id is open: drawn at 3 and 4 tokens, ignored below the minimum, the state stays; it ends at 5
        assert got[1] == [40, 41, EOS, EOS, EOS]
        assert eng.read_finish(1) == ("stop_token", EOS)
        assert eng.read_constraint_trace(1, 5) == [0, 1, 2, 2, 2]
    eng.set_stop_conditions(False)


def test_allowed_token_ids_at_temperature_one_and_a_half():
    eng = _fresh()
    reqs = [Request([5 + r, 9, 300], 40, allowed_token_ids=ALLOWED, temperature=1.5, top_k=0) for r in range(5)]
    res = ContinuousBatcher(eng, sync_every=8, temperature=0.8, top_k=50).run(reqs)
    drawn = [t for toks in res["tokens"] for t in toks]
    assert len(drawn) == 200 and set(drawn) <= set(ALLOWED)
    assert len(set(drawn)) >= 5, sorted(set(drawn))  # (a hot distribution over the set, not one token)


def test_refusals():
    eng = _fresh(False)
    with pytest.raises(RuntimeError, match=r"constraints are off \(set_constraints\)"):
        eng.admit(0, [1, 2], 3, None, 1, **KW, constraint="set")
    with pytest.raises(RuntimeError, match=r"constraints are off \(set_constraints\)"):
        eng.register_constraint("set", Automaton.from_allowed(ALLOWED))
    with pytest.raises(RuntimeError, match="off"):
        eng.read_constraint_trace(0, 1)
    eng.admit(0, [1, 2], 1, None, 1, **KW, constraint=None)  # spelled-out "none" needs nothing
    eng.set_constraints(True)
    eng.register_constraint("set", Automaton.from_allowed(ALLOWED))
    eng.register_constraint("pick", Automaton.from_choices(CHOICES))
    with pytest.raises(ValueError, match="registered already"):
        eng.register_constraint("set", Automaton.from_allowed([1]))
    with pytest.raises(ValueError, match="token 512 is outside the vocabulary 0..511"):
        eng.register_constraint("wide", Automaton.from_allowed([512]))
    with pytest.raises(ValueError, match="temperature <= 100"):
        eng.admit(0, [1, 2], 3, None, 1, temperature=150.0, top_k=50, constraint="set")
    with pytest.raises(ValueError, match="dead end.*no EOS id"):
        eng.admit(0, [1, 2], 3, None, 1, **KW, constraint="pick")      # choices without an EOS id
    with pytest.raises(ValueError, match="an edge names the request's EOS id 64"):
        eng.admit(0, [1, 2], 3, 64, 1, **KW, constraint="set")          # checked against the request's own EOS id
    with pytest.raises(ValueError, match="unknown constraint 'nope'"):
        eng.admit(0, [1, 2], 3, None, 1, **KW, constraint="nope")
    assert eng.read_state()[SLOT_ACTIVE] == 0  # refused before anything moved
    with pytest.raises(ValueError, match="request 0: choices need an EOS id"):
        ContinuousBatcher(eng, **KW).run([Request([1, 2], 3, choices=CHOICES)])
    eng.admit(1, [1, 2], 6, None, 1, **KW, constraint="set")
    with pytest.raises(RuntimeError, match="idle"):
        eng.set_constraints(False)
    with pytest.raises(RuntimeError, match="constraint 'set' is in use by slot 1"):
        eng.drop_constraint("set")
    eng.drop_constraint("pick")  # nobody names it
    assert not eng.has_constraint("pick") and eng.has_constraint("set")
    eng.run_steps(6, **KW)
    eng.drop_constraint("set")   # the finished slot lets go
    with pytest.raises(ValueError, match="unknown constraint 'set'"):
        eng.drop_constraint("set")
    # the engines without admission and EOS word refuse the setter with the reason
    m, ths = _model("tiny-test", None, 1)
    for other in (DecodeEngine(m, ths), BatchedDecodeEngine(m, ths, 1)):
        with pytest.raises(NotImplementedError, match="has no constrained decoding.*only SlotDecodeEngine"):
            other.set_constraints(True)
        other.set_constraints(False)


def test_generate_requests_end_to_end_with_constraints_and_choices(tmp_path):
    f, c = tmp_path / "reqs.jsonl", tmp_path / "cons.jsonl"
    yn = Automaton.from_choices([[100, 101], [200]])
    c.write_text(json.dumps({"id": "yn", **yn.to_json()}) + "\n" +
                 json.dumps({"id": "not-these", "states": [{"edges": [[t, -1] for t in range(0, 512, 2) if t != EOS], "default": 0, "accept": True}]}) + "\n")
    f.write_text('{"tokens": [1, 2, 3], "constraint": "yn", "seed": 3}\n'
                 '{"tokens": [4], "max_new_tokens": 20, "seed": 5}\n'
                 f'{{"tokens": [5, 6, 7, 8, 9], "choices": {json.dumps(CHOICES)}, "seed": 7}}\n'
                 '{"tokens": [10, 11], "max_new_tokens": 9, "allowed_token_ids": [3, 17, 64], "seed": 8}\n'
                 '{"tokens": [10, 12], "max_new_tokens": 30, "constraint": "not-these", "seed": 9}\n')
    args = ("--compile", "--requests", str(f), "--batch_size", "2", "--sparsity", "0.0", "--eos_id", str(EOS))
    res = _main(*args, "--constraints", str(c))
    seqs = res["sequences"]
    assert seqs[0] in ([100, 101, EOS], [200, EOS])
    assert seqs[2][-1] == EOS and seqs[2][:-1] in CHOICES
    # (from_allowed's one state accepts, so under --eos_id the request may also end on the EOS id — and only end on it)
    assert (len(seqs[3]) == 9 or seqs[3][-1] == EOS) and set(seqs[3][:-1]) <= {3, 17, 64} and seqs[3][-1] in (3, 17, 64, EOS)
    assert all(t % 2 == 1 or t == EOS for t in seqs[4]) and (len(seqs[4]) == 30 or seqs[4][-1] == EOS)  # "anything but the even ids"
    only = tmp_path / "only.jsonl"
    only.write_text('{"tokens": [4], "max_new_tokens": 20, "seed": 5}\n')
    assert _main("--compile", "--requests", str(only), "--batch_size", "2", "--sparsity", "0.0", "--eos_id", str(EOS))["sequences"][0] == seqs[1]
    with pytest.raises(SystemExit, match=r'request line 1: "choices" needs an EOS id'):
        only.write_text('{"tokens": [4], "choices": [[1]]}\n')
        _main("--compile", "--requests", str(only), "--batch_size", "2", "--sparsity", "0.0")
    with pytest.raises(SystemExit, match=r"--constraints: constraint 'yn': state 0: token 600 is outside the vocabulary 0..511"):
        c.write_text('{"id": "yn", "states": [{"edges": [[600, 0]], "accept": true}]}\n')
        only.write_text('{"tokens": [4], "constraint": "yn"}\n')
        _main(*args[:1], "--requests", str(only), *args[3:], "--constraints", str(c))


def test_with_the_feature_off_a_step_and_an_admission_launch_what_they_launched():
    B = 3
    m, ths = _model("tiny-test", None, B, max_seq=MAX_SEQ)
    eng = SlotDecodeEngine(m, ths, B)

    def admit_all(**kw):
        for s, (p, b, seed) in REQS3.items():
            eng.admit(s, p, b, None, seed, **KW, **kw)

    step = lambda: eng._self_step(**KW)  # noqa: E731
    admit = lambda: eng.admit(0, [1, 2, 3], 2, None, 5, **KW)  # noqa: E731
    admit_all()
    fresh = _calls(eng, step)
    n_layers = len(m.layers)
    # embedding rows; per layer qkv, attention, wo, resid, gate|up, down, resid; lm_head and its rounding; B samplers; retire
    assert len(fresh) == 1 + 7 * n_layers + 2 + B + 1 and "teal_constrain_logits" not in fresh
    eng.run_steps(BUDGET, use_graph=False, **KW)
    admit_fresh = _calls(eng, admit)
    assert "teal_constrain_logits" not in admit_fresh
    eng.run_steps(2, use_graph=False, **KW)
    eng.set_constraints(True)
    eng.register_constraint("set", Automaton.from_allowed(ALLOWED))
    admit_all(constraint="set")
    on = _calls(eng, step)
    at = on.index("teal_constrain_logits")
    assert on[:at] + on[at + 1:] == fresh and on[at + 1:] == ["teal_sample_topk_slot"] * B + ["teal_batched_retire"]  # one launch, all rows
    eng.run_steps(BUDGET, use_graph=False, **KW)
    admit_on = _calls(eng, admit)
    at = admit_on.index("teal_constrain_logits")
    assert admit_on[:at] + admit_on[at + 1:] == admit_fresh and admit_on[at + 1:] == ["teal_sample_topk_slot", "teal_batched_retire"]
    eng.run_steps(2, use_graph=False, **KW)
    eng.set_constraints(False)
    admit_all()
    assert _calls(eng, step) == fresh and eng._con is None
    eng.run_steps(BUDGET, use_graph=False, **KW)
    assert _calls(eng, admit) == admit_fresh
