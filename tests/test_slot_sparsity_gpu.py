"""GPU: per-request sparsity through SlotDecodeEngine (set_slot_sparsity, admit(..., thresholds=), kept_by_slot) on `tiny-test` and
`tiny-gqa-test`, MAX_SEQ = 64.  The engine is built at level B = 0.5; level A = 0.3 and "dense" (every row kept) are other
threshold sets of the same weights.  Prompts have 2..16 tokens: their prompt pass is the dense HIP pass, which no threshold enters.

  1. feature on with every slot at the default level: tokens and logits bit-identical to feature off, over 32 graph replays;
  2. ONE active slot admitted at level A on the engine built at B draws the tokens of a second engine built at A, bit for bit
     (the union is then that slot's own rows, so the rows' dealing to waves — the order of the sums — is the same);
  3. one captured graph serves admissions at different levels (the graph object's identity), and kept_by_slot follows each;
  4. a dense slot next to a sparse one keeps every row in every launch while the sparse one keeps its own share;
  5. a slot re-admitted without `thresholds` runs at the default: its whole column is rewritten;
  6. with the feature off a step launches what it launched before; on, the layers' GEMMs are the new entry and the lm_head is not;
  7. the setter's and the admission's refusals;
  8. a refused admission has written nothing: the threshold table, the constraint rows and the stop table are bit-equal;
  9. generate.py --requests end to end on a file that mixes levels.
"""
import functools
import math

import pytest
import torch

from teal_amd.gpt_fast.batched import PROJ_KEYS, SLOT_ACTIVE, SLOT_PRODUCED, BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.constraints import Automaton
from teal_amd.gpt_fast.engine import DecodeEngine
from teal_amd.gpt_fast.score import dense_thresholds
from test_logit_engine_gpu import _calls_of, _main, _model

pytestmark = pytest.mark.gpu
MAX_SEQ, B = 64, 3
MODELS = ("tiny-test", "tiny-gqa-test")
KW = dict(temperature=0.8, top_k=50)
REQS = {0: ([5, 9, 300, 9, 17], 40, 21), 1: ([44, 3], 40, 22), 2: ([7, 7, 7, 450, 2, 2, 81, 6, 13, 250, 11], 40, 23)}


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(engine at level B with 3 slots, thresholds at B, at A, dense)"""
    m, ths_b = _model(name, None, B, max_seq=MAX_SEQ, sparsity=0.5)
    _, ths_a = _model(name, None, 1, max_seq=MAX_SEQ, sparsity=0.3)  # the same seed: the same weights, another level
    return SlotDecodeEngine(m, ths_b, B), ths_b, ths_a, dense_thresholds(ths_b)


def _drain(eng):
    while eng.read_state()[SLOT_ACTIVE]:
        eng.run_steps(8, **KW)


def _replays(eng, reqs, n, ths=None):
    """admit, then n graph replays one by one -> (tokens per slot, the logits after each replay)"""
    for s, (prompt, budget, seed) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **KW, **({"thresholds": ths[s]} if ths and ths.get(s) is not None else {}))
    logits = []
    for _ in range(n):
        eng.run_steps(1, **KW)
        logits.append(eng.logits.clone())
    st = eng.read_state()
    toks = {s: eng.read_history(s, st[SLOT_PRODUCED + s]) for s in reqs}
    _drain(eng)
    return toks, torch.stack(logits)


@pytest.mark.parametrize("name", MODELS)
def test_on_at_the_default_level_is_off_bit_for_bit(name):
    eng, ths_b, _, _ = _setup(name)
    eng.set_slot_sparsity(False)
    off_t, off_l = _replays(eng, REQS, 32)
    eng.set_slot_sparsity(True)
    assert eng.tau_table.shape == (len(ths_b), 4, 3, 8) and eng.tau_table.dtype == torch.float32 and eng.tau_table.data_ptr() % 32 == 0
    on_t, on_l = _replays(eng, REQS, 32)
    eng.set_slot_sparsity(False)
    assert all(len(off_t[s]) == 33 for s in REQS) and on_t == off_t
    assert torch.equal(on_l.view(torch.int16), off_l.view(torch.int16))


@pytest.mark.parametrize("name", MODELS)
def test_one_slot_at_another_level_is_an_engine_built_at_that_level(name):
    eng, ths_b, ths_a, _ = _setup(name)
    assert any(ths_a[i][p] != ths_b[i][p] for i in range(len(ths_b)) for p in PROJ_KEYS)
    one = {1: REQS[1]}
    eng.set_slot_sparsity(True)
    got_t, got_l = _replays(eng, one, 32, ths={1: ths_a})
    at_b, _ = _replays(eng, one, 32)
    eng.set_slot_sparsity(False)
    m2, ths_a2 = _model(name, None, B, max_seq=MAX_SEQ, sparsity=0.3)
    assert ths_a2 == ths_a
    ref = SlotDecodeEngine(m2, ths_a, B)
    want_t, want_l = _replays(ref, one, 32)
    assert got_t == want_t and torch.equal(got_l[:, 1].view(torch.int16), want_l[:, 1].view(torch.int16))
    assert at_b != want_t, "levels A and B draw the same tokens: the comparison shows nothing"


@pytest.mark.parametrize("name", MODELS)
def test_one_graph_serves_every_level_and_kept_follows_the_admissions(name):
    eng, ths_b, ths_a, dense = _setup(name)
    nothing = [{p: math.inf for p in PROJ_KEYS} for _ in ths_b]
    eng.set_slot_sparsity(True)
    prompt, budget, seed = REQS[0]
    eng.admit(0, prompt, budget, None, seed, **KW, thresholds=dense)
    eng.admit(1, *REQS[1][:2], None, REQS[1][2], **KW)
    eng.run_steps(2, **KW)
    graph = eng._graph
    assert graph is not None
    k = eng.kept_by_slot()
    assert set(k) == set(PROJ_KEYS) and all(len(v) == B for v in k.values())
    # a dense slot next to a sparse one: every row in every launch; the sparse one its own share; the idle slot nothing
    assert all(k[p][0] == 1.0 for p in PROJ_KEYS), k
    assert all(0.2 < k[p][1] < 0.8 for p in PROJ_KEYS), k
    assert all(k[p][2] == 0.0 for p in PROJ_KEYS)
    assert eng.kept_fractions()["q"]["union"] == 1.0
    alone_b = dict(k)
    _drain(eng)
    # the same slots the other way round, a third at a level that keeps nothing: the same graph object
    eng.admit(0, prompt, budget, None, seed, **KW, thresholds=ths_a)
    eng.admit(1, *REQS[1][:2], None, REQS[1][2], **KW, thresholds=dense)
    eng.admit(2, *REQS[2][:2], None, REQS[2][2], **KW, thresholds=nothing)
    eng.run_steps(2, **KW)
    assert eng._graph is graph
    k = eng.kept_by_slot()
    assert all(k[p][1] == 1.0 and k[p][2] == 0.0 for p in PROJ_KEYS), k
    assert all(alone_b[p][1] < k[p][0] < 1.0 for p in ("q", "gate", "down")), (k, alone_b)  # level 0.3 keeps more than level 0.5
    _drain(eng)
    # re-admitted without thresholds: the default level again, the whole column rewritten (slot 1 was dense, slot 2 kept nothing)
    for s in (1, 2):
        eng.admit(s, *REQS[s][:2], None, REQS[s][2], **KW)
    eng.run_steps(2, **KW)
    assert eng._graph is graph
    fresh = SlotDecodeEngine._tau_column(ths_b)
    for s in (1, 2):
        assert torch.equal(eng.tau_table[..., s].cpu(), torch.tensor(fresh, dtype=torch.float32))
    k = eng.kept_by_slot()
    assert all(0.2 < k[p][s] < 0.8 for p in PROJ_KEYS for s in (1, 2)), k
    assert all(abs(k[p][1] - alone_b[p][1]) < 0.1 for p in PROJ_KEYS), (k, alone_b)
    _drain(eng)
    eng.set_slot_sparsity(False)
    assert eng.tau_table is None and eng._graph is None


def test_off_launches_what_it_launched_and_on_swaps_the_layer_gemms():
    eng, ths_b, _, _ = _setup("tiny-test")
    n_layers = len(ths_b)
    eng.set_slot_sparsity(False)
    step = lambda: eng._self_step(**KW)  # noqa: E731
    off = _calls_of(eng, step)
    assert off.count("teal_batched_sparse_gemm_slots") == 4 * n_layers + 1 and "teal_batched_sparse_gemm_slot_taus" not in off
    eng.set_slot_sparsity(True)
    on = _calls_of(eng, step)
    assert on.count("teal_batched_sparse_gemm_slot_taus") == 4 * n_layers and on.count("teal_batched_sparse_gemm_slots") == 1
    assert [c.replace("_slot_taus", "_slots") for c in on] == off
    eng.set_slot_sparsity(False)
    assert _calls_of(eng, step) == off
    torch.cuda.synchronize()


def test_refusals():
    eng, ths_b, ths_a, _ = _setup("tiny-test")
    eng.set_slot_sparsity(False)
    prompt, budget, seed = REQS[0]
    with pytest.raises(RuntimeError, match="per-request sparsity is off"):
        eng.admit(0, prompt, budget, None, seed, **KW, thresholds=ths_a)
    assert eng.read_state()[SLOT_ACTIVE] == 0
    eng.set_slot_sparsity(True)
    bad_nan = [dict(t) for t in ths_a]
    bad_nan[1]["gate"] = math.nan
    bad_key = [dict(t) for t in ths_a]
    del bad_key[0]["down"]
    for bad, why in ((bad_nan, "NaN"), (ths_a[:1], "one per layer"), (bad_key, "no 'down'")):
        with pytest.raises(ValueError, match=why):
            eng.admit(0, prompt, budget, None, seed, **KW, thresholds=bad)
    assert eng.read_state()[SLOT_ACTIVE] == 0
    eng.admit(0, prompt, budget, None, seed, **KW, thresholds=ths_a)
    for on in (True, False):
        with pytest.raises(RuntimeError, match="idle engine"):
            eng.set_slot_sparsity(on)
    _drain(eng)
    eng.set_slot_sparsity(False)
    # the engines without admissions refuse with that reason; off is what they are
    m, ths = _model("tiny-test", None, 2, max_seq=MAX_SEQ)
    for other in (BatchedDecodeEngine(m, ths, 2), DecodeEngine(_model("tiny-test", None, 1, max_seq=MAX_SEQ)[0], ths)):
        other.set_slot_sparsity(False)
        with pytest.raises(NotImplementedError, match="admission"):
            other.set_slot_sparsity(True)


def test_a_refused_admission_leaves_the_slot_as_it_found_it():
    """admit refuses before its first write to a device table: with slot sparsity, constraints, stop conditions and logit
    processors on and per-request sampling off, neither the "sampling is off" refusal (it used to come after the slot's threshold
    column and constraint row were written) nor one of the logit processors' changes the threshold table, the constraint rows or
    the stop table by a bit, and the slot stays free"""
    _, _, ths_a, _ = _setup("tiny-test")
    m, ths = _model("tiny-test", None, 2, max_seq=MAX_SEQ, sparsity=0.5)
    eng = SlotDecodeEngine(m, ths, 2)
    eng.set_slot_sparsity(True)
    eng.set_constraints(True)
    eng.set_stop_conditions(True)
    eng.set_logit_processors(True)
    eng.register_constraint("yn", Automaton.from_allowed([1, 2]))
    assert eng._samp is None

    def snapshot():
        return eng.tau_table.clone(), list(eng._con.row_names), eng.stop_table.clone()
    before = snapshot()
    prompt, budget, seed = REQS[0]
    refused = ((RuntimeError, "per-request sampling is off", dict(thresholds=ths_a, constraint="yn", top_p=0.9)),
               (ValueError, "logit_bias: token id", dict(stop_token_ids=[1], logit_bias={str(eng.cfg.vocab_size): 1.0})))
    for exc, why, kw in refused:
        with pytest.raises(exc, match=why):
            eng.admit(1, prompt, budget, None, seed, **KW, **kw)
        after = snapshot()
        assert torch.equal(after[0].view(torch.int32), before[0].view(torch.int32)) and after[1] == before[1]
        assert torch.equal(after[2], before[2])
        assert eng.read_state()[SLOT_ACTIVE] == 0


def test_generate_requests_end_to_end_with_mixed_levels(tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text('{"tokens": [1, 2, 3], "sparsity": 0.0}\n'
                 '{"tokens": [4, 5], "max_new_tokens": 20}\n'
                 '{"tokens": [5, 6, 7, 8, 9], "max_new_tokens": 9, "sparsity": 0.3}\n'
                 '{"tokens": [10, 11], "max_new_tokens": 16, "sparsity": 0.5}\n')
    res = _main("--compile", "--requests", str(f), "--batch_size", "2", "--sync_every", "2")
    assert [len(s) for s in res["sequences"]] == [12, 20, 9, 16]
    k = res["kept_by_request"]
    assert k[0] == 1.0 and all(0.05 < k[r] < 1.0 for r in (1, 2, 3)), k
    assert k[2] > k[3]  # level 0.3 keeps more rows than level 0.5
    # a file whose levels are all the run's own leaves the feature off: no report, the parent's launches
    f.write_text('{"tokens": [1, 2, 3], "sparsity": 0.5}\n{"tokens": [4, 5]}\n')
    assert "kept_by_request" not in _main("--compile", "--requests", str(f), "--batch_size", "2")
