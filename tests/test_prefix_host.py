"""CPU: shared prompt prefixes of continuous batching (teal_prefix.hip, continuous.py, generate.py --prefixes) — what needs no GPU.

  * teal_kv_copy_rows is exported and declared, and its unit builds for gfx950 with the library's flags, no scratch, no spills;
  * parse_prefixes / parse_requests with prefixes: the accepted forms and every refusal; cache_rows counts the prefix;
  * ContinuousBatcher against a fake engine that records admit calls: prefix requests arrive as (prefix=name, suffix tokens),
    plain ones exactly as before, registration once per prefix and before the first admission, FIFO order and streams unchanged,
    an oversize prefix + suffix + budget refused before anything runs;
  * generate.py's refusals: --prefixes without --requests, an unknown prefix id in the request file.
"""
import os
import re

import pytest

from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request, cache_rows, parse_prefixes, parse_requests
from test_continuous_host import FakeEngine, _args, _expected, _resources


def test_kv_copy_rows_is_exported_and_declared():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    assert "teal_kv_copy_rows" in _lib.EXPORTS and re.search(r"\bteal_kv_copy_rows\(", hdr)
    assert "teal_prefix.hip" in _lib.SOURCES


def test_prefix_kernels_do_not_spill_to_scratch(tmp_path):
    res = _resources(tmp_path, "teal_prefix.hip")
    assert len(res) >= 1 and any("kv_copy_rows" in n for n in res), sorted(res)
    assert all(v == (0, 0) for v in res.values()), res


class Tok:
    def bos_id(self):
        return 1

    def encode(self, s):
        return [ord(c) for c in s]


def test_parse_prefixes():
    pf = parse_prefixes(['{"id": "sys", "tokens": [1, 2, 3]}', "", '{"id": "shots", "prompt": "ab"}'], Tok())
    assert pf == {"sys": [1, 2, 3], "shots": [1, ord("a"), ord("b")]}
    assert list(pf) == ["sys", "shots"]  # file order: the order they are registered in
    assert parse_prefixes([]) == {}
    for bad, msg in [('{"id": "a", "prompt": "hi"}', "tokenizer"), ('{"id": "a", "tokens": []}', "non-empty"),
                     ('{"id": "a", "tokens": [1], "prompt": "x"}', "exactly one"), ('{"id": "a"}', "exactly one"),
                     ('{"tokens": [1]}', "\"id\""), ('{"id": 3, "tokens": [1]}', "\"id\""), ("not json", "not JSON"),
                     ('{"id": "a", "tokens": [-1]}', "token ids"), ("[1, 2]", "\"id\"")]:
        with pytest.raises(ValueError, match=msg):
            parse_prefixes([bad])
    with pytest.raises(ValueError, match=r"prefix line 3: duplicate id 'a'"):
        parse_prefixes(['{"id": "a", "tokens": [1]}', '{"id": "b", "tokens": [1]}', '{"id": "a", "tokens": [2]}'])
    with pytest.raises(ValueError, match="prefix line 2"):
        parse_prefixes(['{"id": "a", "tokens": [1]}', "{"])


def test_parse_requests_with_prefixes():
    pf = {"sys": [1, 7, 8, 9]}
    lines = ['{"tokens": [4, 5], "prefix": "sys"}', '{"tokens": [6]}', '{"prompt": "hi", "prefix": "sys", "max_new_tokens": 3}',
             '{"prompt": "hi"}']
    rs = parse_requests(lines, 20, Tok(), eos_id=2, prefixes=pf)
    assert [(r.tokens, r.max_new_tokens, r.eos_id, r.prefix) for r in rs] == [
        ([4, 5], 20, 2, "sys"), ([6], 20, 2, None),
        ([ord("h"), ord("i")], 3, 2, "sys"),        # under a prefix: no BOS, the prefix holds it
        ([1, ord("h"), ord("i")], 20, 2, None)]     # without one: BOS prepended, as before
    with pytest.raises(ValueError, match=r"request line 2: unknown prefix 'nope'"):
        parse_requests(['{"tokens": [1]}', '{"tokens": [1], "prefix": "nope"}'], 5, prefixes=pf)
    with pytest.raises(ValueError, match=r"request line 1: unknown prefix 'sys'"):
        parse_requests(['{"tokens": [1], "prefix": "sys"}'], 5)
    with pytest.raises(ValueError, match="non-empty"):
        parse_requests(['{"tokens": [], "prefix": "sys"}'], 5, prefixes=pf)
    with pytest.raises(ValueError, match="empty suffix"):
        parse_requests(['{"prompt": "", "prefix": "sys"}'], 5, Tok(), prefixes=pf)


def test_request_keeps_its_positional_fields():
    r = Request([1, 2], 5, 9, 77)
    assert (r.tokens, r.max_new_tokens, r.eos_id, r.seed, r.prefix) == ([1, 2], 5, 9, 77, None)
    assert Request([1], 2, prefix="a").prefix == "a" and Request([1], 2, None, None, "b").prefix == "b"


def test_cache_rows_counts_the_prefix():
    pf = {"a": [1] * 20, "b": [1] * 50}
    reqs = [Request([1] * 5, 10), Request([1] * 3, 4, prefix="a"), Request([1] * 2, 6, prefix="b")]
    assert cache_rows(reqs, 128, pf) == 58
    assert cache_rows(reqs[:2], 128, pf) == 27
    with pytest.raises(ValueError, match="block_size"):
        cache_rows(reqs, 57, pf)
    with pytest.raises(ValueError, match="unknown prefix"):
        cache_rows(reqs, 128)
    assert cache_rows([Request([1] * 5, 10), Request([1] * 30, 3)], 128) == 33  # as before


class PrefixFakeEngine(FakeEngine):
    """FakeEngine with the prefix interface; records what admit and register_prefix were called with"""

    def __init__(self, B=4, max_seq=64):
        super().__init__(B, max_seq)
        self.registered, self.calls, self.events = {}, [], []
        self.prefix_paths = {"hip": 0, "module": 0}

    def has_prefix(self, name):
        return name in self.registered

    def register_prefix(self, name, tokens):
        assert name not in self.registered and self.state[0] == 0
        self.registered[name] = list(tokens)
        self.events.append(("register", name))
        return len(tokens)

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        assert set(kw) <= {"prefix"}
        if "prefix" in kw:
            assert kw["prefix"] in self.registered
            self.prefix_paths["hip"] += 1
        self.calls.append((list(tokens), budget, seed, dict(kw)))
        self.events.append(("admit", seed))
        P = len(self.registered[kw["prefix"]]) if "prefix" in kw else 0
        super().admit(slot, [0] * P + list(tokens), budget, eos_id, seed, temperature, top_k)


PF = {"sys": [1, 2, 3, 4, 5, 6], "shots": [9] * 11}
PREQS = [Request([1, 2, 3], 5), Request([7, 8], 17, prefix="sys"), Request([4], 3, prefix="shots"), Request([1, 2, 3], 9),
         Request([5, 5, 5], 1, prefix="sys"), Request([6], 12), Request([2, 2], 7, prefix="shots"), Request([3], 2, prefix="sys"),
         Request([1, 2], 20), Request([8, 9], 4, prefix="sys")]


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("refill", ["free", "all"])
def test_batcher_passes_prefix_and_suffix(K, refill):
    eng = PrefixFakeEngine()
    res = ContinuousBatcher(eng, sync_every=K, refill=refill, prefixes=PF).run(PREQS)
    # FIFO: call r is request r, with its own stream seed + r
    assert [(t, b, s) for t, b, s, _ in eng.calls] == [(q.tokens, q.max_new_tokens, 1234 + r) for r, q in enumerate(PREQS)]
    # a prefix request arrives with prefix=name and its suffix only; a plain one with no such keyword at all
    assert [kw for *_, kw in eng.calls] == [({"prefix": q.prefix} if q.prefix is not None else {}) for q in PREQS]
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(PREQS)]
    n = sum(q.prefix is not None for q in PREQS)
    assert res["prefix_admissions"] == n and res["admissions"] == len(PREQS)
    assert res["prefix_rows_reused"] == sum(len(PF[q.prefix]) for q in PREQS if q.prefix is not None)
    assert res["prefix_paths"] == {"hip": n, "module": 0}


def test_prefixes_are_registered_once_and_before_the_first_admission():
    eng = PrefixFakeEngine()
    b = ContinuousBatcher(eng, sync_every=2, prefixes=PF)
    b.run(PREQS)
    assert eng.events[:2] == [("register", "sys"), ("register", "shots")] and eng.events[2][0] == "admit"
    assert eng.registered == PF
    b.run(PREQS)  # a second run on the same engine registers nothing again
    assert [e for e in eng.events if e[0] == "register"] == [("register", "sys"), ("register", "shots")]
    # an engine that holds one of them already gets only the other
    eng2 = PrefixFakeEngine()
    eng2.register_prefix("shots", PF["shots"])
    ContinuousBatcher(eng2, prefixes=PF).run(PREQS)
    assert [e for e in eng2.events if e[0] == "register"] == [("register", "shots"), ("register", "sys")]


def test_plain_engine_and_plain_requests_are_untouched():
    # the FakeEngine of test_continuous_host.py has no prefix interface: without prefixes nothing of it is asked for
    plain = [q for q in PREQS if q.prefix is None]
    eng = FakeEngine()
    res = ContinuousBatcher(eng, sync_every=3).run(plain)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(plain)]
    assert res["prefix_admissions"] == 0 and res["prefix_rows_reused"] == 0 and res["prefix_paths"] == {}
    # plain requests on a batcher that has prefixes: admitted without the keyword
    eng = PrefixFakeEngine()
    ContinuousBatcher(eng, prefixes=PF).run(plain)
    assert all(kw == {} for *_, kw in eng.calls) and len(eng.registered) == 2


def test_oversize_prefix_requests_are_refused_before_anything_runs():
    eng = PrefixFakeEngine(max_seq=24)
    with pytest.raises(ValueError, match="11 prefix tokens.*do not fit"):
        ContinuousBatcher(eng, prefixes=PF).run([Request([1] * 4, 8), Request([1] * 6, 8, prefix="shots")])  # 11 + 6 + 8 = 25
    assert eng.events == [] and eng.reads == 0
    ContinuousBatcher(eng, prefixes=PF).run([Request([1] * 5, 8, prefix="shots")])  # 24 rows: fits
    eng = PrefixFakeEngine()
    with pytest.raises(ValueError, match="unknown prefix 'nope'"):
        ContinuousBatcher(eng, prefixes=PF).run([Request([1], 2, prefix="nope")])
    with pytest.raises(ValueError, match="unknown prefix 'sys'"):
        ContinuousBatcher(eng).run([Request([1], 2, prefix="sys")])
    assert eng.events == [] and eng.reads == 0


def test_generate_refuses_prefixes_without_requests(tmp_path):
    p = tmp_path / "p.jsonl"
    p.write_text('{"id": "sys", "tokens": [1, 2]}\n')
    with pytest.raises(SystemExit, match="--prefixes.*--requests"):
        G.main(_args("--synthetic", "tiny-test", "--prefixes", str(p)))


def test_generate_refuses_an_unknown_prefix_id(tmp_path):
    p, f = tmp_path / "p.jsonl", tmp_path / "r.jsonl"
    p.write_text('{"id": "sys", "tokens": [1, 2]}\n')
    f.write_text('{"tokens": [1, 2], "prefix": "sys"}\n{"tokens": [3], "prefix": "other"}\n')
    with pytest.raises(SystemExit, match=r"request line 2: unknown prefix 'other'"):
        G.main(_args("--synthetic", "tiny-test", "--batch_size", "4", "--requests", str(f), "--prefixes", str(p)))
    with pytest.raises(SystemExit, match=r"request line 1: unknown prefix 'sys'"):
        G.main(_args("--synthetic", "tiny-test", "--batch_size", "4", "--requests", str(f)))


def test_prefixes_flag_defaults_off():
    assert _args().prefixes is None
