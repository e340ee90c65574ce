"""CPU: per-request sparsity — what needs no GPU.

  * the new entry point is exported, declared and loaded with its signature; its instantiations of batched_gemm_kernel build for
    gfx950 with no scratch and no VGPR spills (the compiler's resource remarks, as tests/test_continuous_host.py reads them);
  * "sparsity" in a request line: parsed, and refused out of range, as more than 8 distinct levels, in a prefix line and — by
    generate.py, before anything is loaded — at a level the run's threshold source cannot serve;
  * ContinuousBatcher against a fake engine: the feature is switched on exactly when some request's level differs from the run's,
    only those requests are admitted with `thresholds=`, and the result reports what each request kept.
"""
import os
import re

import pytest

from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE
from teal_amd.gpt_fast.continuous import (MAX_LEVELS, ContinuousBatcher, Request, check_sparsity_fields, parse_prefixes, parse_requests,
                                          sparsity_levels_of)
from test_continuous_host import FakeEngine, _args, _expected, _resources

NAME = "teal_batched_sparse_gemm_slot_taus"


def test_entry_point_is_exported_declared_and_typed():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    assert NAME in _lib.EXPORTS and NAME in _lib.OPTIONAL_WITH_OVERRIDE and re.search(rf"\b{NAME}\(", hdr)
    decl = re.search(rf"int {NAME}\((.*?)\);", hdr, re.S).group(1)
    slots = re.search(r"int teal_batched_sparse_gemm_slots\((.*?)\);", hdr, re.S).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]  # noqa: E731
    assert [a for a in norm(decl) if a != "const float* taus"] == norm(slots) and "const float* taus" in norm(decl)
    src = open(os.path.join(_lib.CSRC, "teal_batched.hip")).read()
    assert re.search(rf"\bint {NAME}\(", src)
    if os.path.exists(_lib.LIB_PATH):  # (a built tree: the symbol is there and the loader knows its 18 arguments)
        L = _lib.load()
        assert len(getattr(L, NAME).argtypes) == len(L.teal_batched_sparse_gemm_slots.argtypes) + 1


def test_slot_taus_instantiations_use_no_scratch(tmp_path):
    res = _resources(tmp_path, "teal_batched.hip")
    taus = {n: v for n, v in res.items() if "batched_gemm_kernel" in n and "ELb1ELb1EEEv" in n}   # <.., TAUS = true, SLOTS = true>
    assert len(taus) == 24, sorted(taus)   # 2 dtypes x 4 slot-pair counts x 3 producers
    assert all(v == (0, 0) for v in taus.values()), {n: v for n, v in taus.items() if v != (0, 0)}
    assert not [n for n in res if "batched_gemm_kernel" in n and "ELb1ELb0EEEv" in n]  # per-slot thresholds without slots: never built


# ---- parsing ----------------------------------------------------------------------------------------------------------------
def test_sparsity_field_is_parsed_and_refused():
    reqs = parse_requests(['{"tokens": [1, 2], "sparsity": 0.0}', '{"tokens": [3]}', '{"tokens": [4], "sparsity": 0.6}'], 5)
    assert [r.sparsity for r in reqs] == [0.0, None, 0.6]
    assert sparsity_levels_of(reqs) == [0.0, 0.6]
    assert Request([1], 2).sparsity is None
    for bad in ("1", "1.0", "-0.1", '"0.5"', "true", "null", "NaN", "[0.5]"):
        with pytest.raises(ValueError, match=r'request line 1: "sparsity" must be a number in \[0, 1\)'):
            parse_requests(['{"tokens": [1], "sparsity": %s}' % bad], 5)
    many = ['{"tokens": [1], "sparsity": %g}' % (0.1 * i) for i in range(MAX_LEVELS + 1)]
    assert MAX_LEVELS == 8 and len(parse_requests(many[:8] + many[:3], 5)) == 11   # 8 distinct levels, repeated: fine
    with pytest.raises(ValueError, match="9 distinct \"sparsity\" levels: at most 8"):
        parse_requests(many, 5)
    with pytest.raises(ValueError, match="9 distinct"):
        check_sparsity_fields(many)
    assert check_sparsity_fields(many[:4] + ["not json", "", '{"tokens": [1]}']) == pytest.approx([0.0, 0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="request line 2: \"sparsity\" 0.7: no such level"):
        check_sparsity_fields(['{"tokens": [1]}', '{"tokens": [1], "sparsity": 0.7}'], lambda lv: "no such level" if lv == 0.7 else None)
    with pytest.raises(ValueError, match="prefix line 1: \"sparsity\" belongs to a request line"):
        parse_prefixes(['{"id": "sys", "tokens": [1, 2], "sparsity": 0.5}'])


def test_generate_refuses_before_anything_is_loaded(tmp_path):
    f = tmp_path / "r.jsonl"
    base = ("--synthetic", "tiny-test", "--batch_size", "2", "--requests", str(f))
    f.write_text('{"tokens": [1, 2], "sparsity": 1.5}\n')
    with pytest.raises(SystemExit, match=r'--requests: request line 1: "sparsity" must be a number in \[0, 1\)'):
        G.main(_args(*base))
    f.write_text("".join('{"tokens": [1], "sparsity": %g}\n' % (0.05 * i) for i in range(9)))
    with pytest.raises(SystemExit, match="--requests: 9 distinct"):
        G.main(_args(*base))
    # a level the chosen source cannot serve: the greedy table holds 0.3 .. 0.6 (level 0 needs no table)
    table = os.path.join(os.path.dirname(__file__), "golden", "greedy_llama2_7b.json")
    f.write_text('{"tokens": [1], "sparsity": 0.5}\n{"tokens": [1], "sparsity": 0.0}\n{"tokens": [1], "sparsity": 0.45}\n')
    with pytest.raises(SystemExit, match=r'request line 3: "sparsity" 0.45: --greedy_lookup .* has no such target'):
        G.main(_args(*base, "--greedy_lookup", table))
    a = _args(*base, "--greedy_lookup", table)
    f.write_text('{"tokens": [1], "sparsity": 0.5}\n{"tokens": [1], "sparsity": 0.0}\n{"tokens": [1]}\n')
    assert G.check_request_sparsity(a) == [0.0, 0.5]
    assert G.check_request_sparsity(_args(*base)) == [0.0, 0.5]   # calibration serves any level


# ---- the batcher's decision -------------------------------------------------------------------------------------------------
class SparseFake(FakeEngine):
    """FakeEngine with the per-request sparsity interface: it records the switch and each admission's thresholds, and a slot
    "keeps" 1 - its level of the rows"""

    def __init__(self, levels, **kw):
        super().__init__(**kw)
        self.switched, self.admitted, self.level = [], [], [None] * self.B
        self.inverse = {id(v): k for k, v in levels.items()}

    def set_slot_sparsity(self, on):
        assert self.state[SLOT_ACTIVE] == 0
        self.switched.append(on)

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, thresholds=None):
        assert thresholds is None or self.switched == [True], "thresholds= with the feature off"
        self.admitted.append((seed, None if thresholds is None else self.inverse[id(thresholds)]))
        self.level[slot] = 0.5 if thresholds is None else self.inverse[id(thresholds)]
        super().admit(slot, tokens, budget, eos_id, seed, temperature, top_k)

    def kept_by_slot(self):
        assert self.switched == [True]
        return {p: [0.0 if lv is None else 1.0 - lv for lv in self.level] for p in ("q", "down")}


LEVELS = {0.0: [{"q": -1.0}], 0.6: [{"q": 9.0}]}


def _reqs(levels):
    return [Request([1, 2, 3], n, sparsity=lv) for n, lv in zip((5, 17, 3, 9, 2, 12, 7), levels)]


@pytest.mark.parametrize("levels", [(None,) * 7, (0.5,) * 7, (None, 0.5, None, 0.5, 0.5, None, None)])
def test_batcher_leaves_the_feature_off_when_every_level_is_the_runs(levels):
    eng = SparseFake(LEVELS)
    reqs = _reqs(levels)
    res = ContinuousBatcher(eng, sync_every=3, sparsity=0.5, sparsity_levels=LEVELS).run(reqs)
    assert eng.switched == [] and all(t is None for _, t in eng.admitted) and "kept_by_request" not in res
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(reqs)]


@pytest.mark.parametrize("K", [1, 3, 8])
def test_batcher_switches_on_and_admits_only_the_other_levels_with_thresholds(K):
    eng = SparseFake(LEVELS)
    levels = (0.6, None, 0.0, 0.5, 0.6, None, 0.0)
    reqs = _reqs(levels)
    b = ContinuousBatcher(eng, sync_every=K, sparsity=0.5, sparsity_levels=LEVELS)
    res = b.run(reqs)
    assert eng.switched == [True]
    assert sorted(eng.admitted) == sorted((1234 + r, lv if lv not in (None, 0.5) else None) for r, lv in enumerate(levels))
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(reqs)]   # the tokens are the requests' own streams either way
    for r, lv in enumerate(levels):  # a request that ran a step a sync point saw reports its own share
        k = res["kept_by_request"][r]
        assert k is None or k == pytest.approx(1.0 - (0.5 if lv is None else lv)), (r, k)
    assert res["kept_by_request"][1] is not None and res["kept_by_request"][5] is not None  # (17 and 12 tokens: seen at any K)
    b.run(reqs)
    assert eng.switched == [True]   # once: a second run keeps the captured step


def test_batcher_refuses_a_level_without_thresholds_before_anything_runs():
    eng = SparseFake(LEVELS)
    with pytest.raises(ValueError, match="request 1: no thresholds for sparsity 0.3"):
        ContinuousBatcher(eng, sparsity=0.5, sparsity_levels=LEVELS).run([Request([1], 2), Request([1], 2, sparsity=0.3)])
    assert eng.switched == [] and eng.admitted == []
    with pytest.raises(ValueError, match="must be a number in"):
        ContinuousBatcher(eng, sparsity=1.0)
    # the run's level unknown: any request that names one differs from it
    eng = SparseFake(LEVELS)
    ContinuousBatcher(eng, sparsity_levels=LEVELS).run([Request([1], 2, sparsity=0.6)])
    assert eng.switched == [True] and eng.admitted == [(1234, 0.6)]
