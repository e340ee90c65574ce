"""CPU: constrained decoding (teal_constrain.hip, constraints.py, continuous.py, generate.py --constraints) — what needs no GPU.

  * Automaton.check refuses every malformed table with its reason; image() is the layout the rule (tests/constraint_rule.py) reads;
  * from_choices walks to exactly the given set (the language up to length 8 is enumerated), from_allowed, the JSON round trip;
  * the arena allocator reuses a freed block, coalesces neighbours and refuses when full;
  * parse_requests reads the new fields and refuses two kinds on one line, "choices" strings without a tokenizer, "choices" without
    an EOS id and an unknown constraint id with the line number; parse_constraints;
  * ContinuousBatcher against a fake engine: the feature is switched on exactly when a request carries a constraint, one automaton
    per distinct content, only constrained requests are admitted with the keyword;
  * generate.py refuses --constraints without --requests and an unknown id before anything is loaded;
  * the header declares teal_constrain_logits, _lib lists the source and the symbol, the unit builds without scratch or spills;
  * the off-state feature key and loop state of SamplerFeatures are unchanged, and only the slot engine takes the setter.
"""
import json
import os
import re

import pytest
import torch

import constraint_rule as R
from teal_amd import _lib
from teal_amd.gpt_fast import constraints as CN
from teal_amd.gpt_fast import engine_features as EF
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.constraints import ArenaAllocator, Automaton
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request, parse_constraints, parse_requests
from test_continuous_host import FakeEngine, _args, _expected, _resources


def S(edges=(), default=-1, accept=False):
    return {"edges": list(edges), "default": default, "accept": accept}


# ---- Automaton ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("states,eos,msg", [
    ([S([(3, 0), (2, 0)])], None, "state 0: tokens must be strictly ascending .*unsorted"),
    ([S([(2, 0), (2, 0)])], None, "state 0: tokens must be strictly ascending .*duplicated"),
    ([S([(16, 0)])], None, "state 0: token 16 is outside the vocabulary 0..15"),
    ([S([(-1, 0)])], None, "state 0: token -1 is outside the vocabulary"),
    ([S([(1, 1)]), S([(2, 2)])], None, "state 1: next 2 of token 2 is outside -1..1"),
    ([S([(1, -2)])], None, "state 0: next -2 of token 1 is outside -1..0"),
    ([S([(1, 0)], default=1)], None, "state 0: default 1 is outside -1..0"),
    ([S([(1, 0)], default=-2)], None, "state 0: default -2 is outside -1..0"),
    ([S([(1, 0), (5, 0)])], 5, "state 0: an edge names the request's EOS id 5"),
    ([S([(1, 1)]), S()], 5, "state 1 is a dead end: no token is allowed and it is not accepting"),
    ([S([(1, 1)]), S([(4, -1)])], 5, "state 1 is a dead end: no token is allowed and it is not accepting"),
    ([S([(1, 1)]), S(accept=True)], None, "state 1 is a dead end: no token is allowed and the request has no EOS id"),
])
def test_check_refuses_with_the_reason(states, eos, msg):
    with pytest.raises(ValueError, match=msg):
        Automaton(states).check(16, eos)


def test_check_accepts_what_is_legal_and_counts_states():
    Automaton([S([(1, 1)]), S(accept=True)]).check(16, 5)                       # only EOS open in state 1
    Automaton([S([(1, 1)]), S(accept=True)]).check(16, None, eos_known=False)   # (a registration: the EOS rules wait for a request)
    with pytest.raises(ValueError, match="state 2 is a dead end"):
        Automaton([S([(1, 1)]), S(accept=True), S()]).check(16, 5)              # unreachable, but a dead end all the same
    Automaton([S([(1, 0)]), S([(2, 1)], accept=True)]).check(16, None)            # an unreachable state is legal
    Automaton([S([(3, -1)], default=0)]).check(16, None)                          # "anything but 3"
    with pytest.raises(ValueError, match="dead end"):                             # everything but the EOS id banned, not accepting
        Automaton([S([(0, -1), (1, -1), (2, -1)], default=0)]).check(4, 3)

    class Many(list):  # (the limit is checked on the count alone: no 2^30 states are built)
        def __len__(self):
            return 2 ** 30

    big = Automaton([S([(1, 0)])])
    big.states = Many(big.states)
    with pytest.raises(ValueError, match="at most 2\\^30 - 1"):
        big.check(16, None)
    for bad in ([], "ab", [3], [S(edges=[(1,)])], [S(edges=[(1.0, 0)])], [S(default=None)], [{"edges": [], "accept": "yes"}]):
        with pytest.raises(ValueError):
            Automaton(bad)


def test_image_is_the_layout_the_rule_reads():
    a = Automaton([S([(2, 1), (9, -1)], default=0), S([(0, 0)], accept=True), S(default=1)])
    img = a.image()
    assert img == R.image([([(2, 1), (9, -1)], 0, False), ([(0, 0)], -1, True), ([], 1, False)])
    assert img[:12] == [12, 16, 0, 0, 16, 18, -1, 1, 18, 18, 1, 0] and img[12:] == [2, 1, 9, -1, 0, 0]
    for s in range(3):
        for t in range(12):
            assert R.delta(img, s, t) == a.delta(s, t)


def _language(a, eos, max_len):
    """every token sequence of at most max_len tokens after which the automaton accepts (the request may end there)"""
    out, frontier = set(), [((), 0)]
    for _ in range(max_len + 1):
        nxt = []
        for seq, s in frontier:
            if a.states[s]["accept"]:
                out.add(seq)
            img = a.image()
            toks = set(t for t, _ in a.states[s]["edges"]) | (set(range(12)) if a.states[s]["default"] >= 0 else set())
            for t in sorted(toks):
                d = R.delta(img, s, t)
                if d >= 0 and t != eos:
                    nxt.append((seq + (t,), d))
        frontier = nxt
    return {q for q in out if len(q) <= max_len}


def test_from_choices_walks_to_exactly_the_given_set():
    choices = [[1, 2, 3], [1, 2], [1, 4], [5], [1, 2, 3, 6, 7, 8, 9, 10], [5], [2, 1]]  # shared prefixes, a prefix of another, a duplicate
    a = Automaton.from_choices(choices).check(12, 11)
    assert _language(a, 11, 8) == {tuple(c) for c in choices}
    assert len(a) == 1 + len({tuple(c[:i]) for c in choices for i in range(1, len(c) + 1)})  # duplicates merged: one node per prefix
    assert all(st["default"] == -1 for st in a.states) and not a.states[0]["accept"]
    with pytest.raises(ValueError, match="dead end.*no EOS id"):
        a.check(12, None)  # its leaves end on the EOS id only
    for bad, msg in (([[1], []], "choice 1 is empty"), ([], "choices is empty"), ([[1, -2]], "not a token id"), ("ab", "list"), ([3], "choice 0")):
        with pytest.raises(ValueError, match=msg):
            Automaton.from_choices(bad)


def test_from_allowed_and_the_json_round_trip():
    a = Automaton.from_allowed([7, 3, 7, 0]).check(8, None)
    assert a.to_json() == {"states": [{"edges": [[0, 0], [3, 0], [7, 0]], "default": -1, "accept": True}]}
    for bad in ([], [1, -1], "12", [True]):
        with pytest.raises(ValueError):
            Automaton.from_allowed(bad)
    b = Automaton([S([(2, 1), (9, -1)], default=0), S([(0, 0)], accept=True), S(default=1)])
    back = Automaton.from_json(b.to_json())
    assert back.image() == b.image() and back.to_json() == b.to_json()
    assert Automaton.from_json(json.loads(json.dumps(b.to_json()))).image() == b.image()
    for bad in ({}, {"states": 3}, [1], {"states": [{"edges": "ab"}]}):
        with pytest.raises(ValueError):
            Automaton.from_json(bad)


# ---- the arena --------------------------------------------------------------------------------------------------------------------
def test_arena_allocator_reuses_coalesces_and_refuses():
    al = ArenaAllocator(64)
    a, b, c, d = al.alloc(16), al.alloc(14), al.alloc(16), al.alloc(16)  # (14 words take a 16-word block: blocks start on 16 bytes)
    assert (a, b, c, d) == (0, 16, 32, 48) and al.free == []
    with pytest.raises(MemoryError, match="arena is full"):
        al.alloc(1)
    al.release(b)
    assert al.alloc(16) == 16  # a freed block is reused (first fit)
    al.release(a)
    al.release(c)
    assert al.free == [(0, 16), (32, 16)]
    with pytest.raises(MemoryError, match="largest free block has 16 of 64"):
        al.alloc(20)  # 32 words free, but not in one piece
    al.release(16)
    assert al.free == [(0, 48)]  # both neighbours coalesced
    assert al.alloc(40) == 0 and al.alloc(8) == 40
    al.release(d)
    al.release(40)
    al.release(0)
    assert al.free == [(0, 64)] and al.used == {}


def test_constraints_buffers_share_images_and_refuse_a_drop_in_use(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)  # (the buffers only keep the handle: nothing is launched here)
    c = CN.Constraints(3, 16, torch.float16, 9, "cpu", capacity_words=64)
    assert c.con.shape == (3, 16) and c.trace.shape == (3, 9) and c.table.tolist() == [[-1, 0, 0, 0]] * 3 and c.arena.numel() == 64
    arena_ptr = c.arena.data_ptr()
    a = Automaton.from_choices([[1, 2], [3]])
    base = c.register("yn", a)
    assert c.arena[base:base + len(a.image())].tolist() == a.image()
    with pytest.raises(ValueError, match="registered already"):
        c.register("yn", a)
    c.set_row(0, "yn")
    c.set_row(2, "yn")
    assert c.table.tolist() == [[base, len(a), 0, 0], [-1, 0, 0, 0], [base, len(a), 0, 0]]  # one image, two slots
    with pytest.raises(RuntimeError, match="in use by slots 0, 2"):
        c.drop("yn")
    with pytest.raises(ValueError, match="unknown constraint 'nope'"):
        c.set_row(1, "nope")
    with pytest.raises(ValueError, match="outside 0..2"):
        c.set_row(3, None)
    c.set_row(0, None)
    c.set_row(2, None)
    c.drop("yn")
    assert c.register("other", Automaton.from_allowed([1])) == base and c.arena.data_ptr() == arena_ptr  # reused, fixed address
    with pytest.raises(MemoryError):
        c.register("big", Automaton([S([(t, 0) for t in range(16)])] * 2))  # 8 + 64 words
    with pytest.raises(ValueError, match="multiple of 8"):
        CN.Constraints(1, 12, torch.float16, 4, "cpu")


# ---- request files ------------------------------------------------------------------------------------------------------------------
class Tok:
    def bos_id(self):
        return 1

    def encode(self, s):
        return [ord(c) for c in s]


def test_parse_requests_reads_the_new_fields():
    cons = parse_constraints(['{"id": "yn", "states": [{"edges": [[4, 1], [5, 1]]}, {"accept": true}]}', ""])
    assert list(cons) == ["yn"] and cons["yn"].to_json()["states"][1] == {"edges": [], "default": -1, "accept": True}
    lines = ['{"tokens": [1], "constraint": "yn"}', '{"tokens": [1], "choices": [[4, 5], [6]]}', '{"tokens": [1], "choices": ["ab", "c"]}',
             '{"tokens": [1], "allowed_token_ids": [9, 3]}', '{"tokens": [1]}']
    rs = parse_requests(lines, 8, Tok(), eos_id=2, constraints=cons)
    assert [(r.constraint, r.choices, r.allowed_token_ids) for r in rs] == [
        ("yn", None, None), (None, [[4, 5], [6]], None), (None, [[ord("a"), ord("b")], [ord("c")]], None),  # strings: alone, no BOS
        (None, None, [9, 3]), (None, None, None)]
    assert rs[4].constraint_spec() is None and rs[0].constraint_spec() == ("yn", None)
    assert rs[1].constraint_spec()[0] == Request([2], 1, 2, choices=[[6], [4, 5], [6]]).constraint_spec()[0]  # keyed by content
    assert rs[3].constraint_spec()[0] == "allowed:[3,9]"


@pytest.mark.parametrize("line,kw,msg", [
    ('{"tokens": [1], "choices": [[1]], "allowed_token_ids": [2]}', {}, r'request line 2: at most one of .* got "choices" and "allowed_token_ids"'),
    ('{"tokens": [1], "constraint": "yn", "choices": [[1]]}', {}, "request line 2: at most one of"),
    ('{"tokens": [1], "choices": ["yes", "no"]}', {"tokenizer": None}, r'request line 2: "choices" strings need a tokenizer'),
    ('{"tokens": [1], "constraint": "nope"}', {}, "request line 2: unknown constraint 'nope'"),
    ('{"tokens": [1], "constraint": "yn"}', {"constraints": None}, r"request line 2: unknown constraint 'yn' \(no constraints were given\)"),
    ('{"tokens": [1], "choices": [[1]]}', {"eos_id": None}, r'request line 2: "choices" needs an EOS id'),
    ('{"tokens": [1], "choices": []}', {}, r'request line 2: "choices" must be'),
    ('{"tokens": [1], "choices": [[1], "a"]}', {}, r'request line 2: "choices" must be'),
    ('{"tokens": [1], "choices": [[]]}', {}, r'request line 2: "choices" must be'),
    ('{"tokens": [1], "allowed_token_ids": []}', {}, r'request line 2: "allowed_token_ids" must be'),
    ('{"tokens": [1], "allowed_token_ids": [1, -1]}', {}, r'request line 2: "allowed_token_ids" must be'),
])
def test_parse_requests_refuses_with_the_line_number(line, kw, msg):
    args = dict(tokenizer=Tok(), eos_id=2, constraints={"yn": Automaton.from_allowed([1])})
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        parse_requests(['{"tokens": [1]}', line], 8, **args)


def test_parse_constraints_refusals():
    for bad, msg in (("{", "constraint line 1: not JSON"), ('{"states": []}', 'constraint line 1: needs an "id"'),
                     ('{"id": "a"}', 'constraint line 1: an automaton object needs "states"'),
                     ('{"id": "a", "states": []}', "constraint line 1: an automaton needs at least one state"),
                     ('{"id": "a", "states": [{"edges": [[1]]}]}', "constraint line 1: state 0: an edge must be")):
        with pytest.raises(ValueError, match=msg):
            parse_constraints([bad])
    with pytest.raises(ValueError, match="constraint line 2: duplicate id 'a'"):
        parse_constraints(['{"id": "a", "states": [{}]}'] * 2)
    assert parse_constraints([]) == {}
    with pytest.raises(ValueError, match="at most one of"):
        Request([1], 2, 3, choices=[[1]], allowed_token_ids=[1])


# ---- the batcher against a fake engine ------------------------------------------------------------------------------------------------
class ConFakeEngine(FakeEngine):
    """FakeEngine with the constraint interface: records what the batcher asks for (the tokens stay the fake's own draws)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.cfg = type("Cfg", (), {"vocab_size": 64})()
        self.events, self.registered, self.kws = [], {}, []

    def set_constraints(self, on, capacity_words=1 << 20):
        assert self.state[0] == 0, "switched on a busy engine"
        self.events.append(("set", on))

    def has_constraint(self, name):
        return name in self.registered

    def register_constraint(self, name, automaton):
        assert name not in self.registered
        self.events.append(("register", name))
        self.registered[name] = automaton

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        self.kws.append(kw)
        self.events.append(("admit", kw.get("constraint")))
        super().admit(slot, tokens, budget, eos_id, seed, temperature, top_k)


def test_batcher_switches_the_feature_on_exactly_when_asked():
    plain = [Request([1, 2], 5), Request([3], 4, eos_id=7)]
    eng = ConFakeEngine()
    res = ContinuousBatcher(eng, sync_every=3, constraints={"yn": Automaton.from_allowed([1, 2])}).run(plain)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(plain)]
    assert all(e[0] == "admit" for e in eng.events) and all(kw == {} for kw in eng.kws)  # no request asks: nothing of it is touched
    ContinuousBatcher(FakeEngine()).run(plain)  # (an engine without the interface serves plain requests as before)

    reqs = [Request([1], 3, eos_id=9, choices=[[4, 5], [6]]), Request([1], 3), Request([1], 3, eos_id=9, choices=[[6], [4, 5]]),
            Request([1], 3, constraint="yn"), Request([1], 3, allowed_token_ids=[2, 1])]
    eng = ConFakeEngine()
    b = ContinuousBatcher(eng, constraints={"yn": Automaton.from_allowed([1, 2]), "unused": Automaton.from_allowed([3])})
    b.run(reqs)
    names = [e[1] for e in eng.events if e[0] == "register"]
    assert eng.events[0] == ("set", True) and eng.events[1:1 + len(names)] == [("register", n) for n in names]  # before the first admission
    assert len(names) == 3 and names[1] == "yn" and names[0].startswith("choices:") and names[2] == "allowed:[1,2]"  # one per distinct content
    assert [e[1] for e in eng.events if e[0] == "admit"] == [names[0], None, names[0], "yn", names[2]]
    assert eng.kws[1] == {}  # the plain request: admitted without the keyword
    b.run(reqs)              # a second run: nothing switched or registered again
    assert [e for e in eng.events if e[0] != "admit"] == [("set", True)] + [("register", n) for n in names]


def test_batcher_refuses_before_anything_runs():
    for reqs, kw, msg in (([Request([1], 3, constraint="nope")], {}, "request 0: unknown constraint 'nope'"),
                          ([Request([1], 3), Request([1], 3, choices=[[1]])], {}, "request 1: choices need an EOS id"),
                          ([Request([1], 3, allowed_token_ids=[64])], {}, "request 0: state 0: token 64 is outside the vocabulary 0..63"),
                          ([Request([1], 3, eos_id=5, allowed_token_ids=[5])], {}, "request 0: state 0: an edge names the request's EOS id 5"),
                          ([Request([1], 3, allowed_token_ids=[1])], {"temperature": 150.0}, "request 0: a constrained request needs temperature <= 100")):
        eng = ConFakeEngine()
        with pytest.raises(ValueError, match=msg):
            ContinuousBatcher(eng, **kw).run(reqs)
        assert eng.events == [] and eng.reads == 0


# ---- generate.py ----------------------------------------------------------------------------------------------------------------------
def test_generate_refuses_constraints_without_requests(tmp_path):
    c = tmp_path / "c.jsonl"
    c.write_text('{"id": "yn", "states": [{"edges": [[1, 0]], "accept": true}]}\n')
    with pytest.raises(SystemExit, match="--constraints.*needs --requests"):
        G.main(_args("--synthetic", "tiny-test", "--constraints", str(c)))
    with pytest.raises(SystemExit, match="--constraints.*needs --requests"):
        G.main(_args("--synthetic", "tiny-test", "--compile", "--batch_size", "4", "--constraints", str(c)))
    assert _args().constraints is None


def test_generate_refuses_an_unknown_constraint_id_before_anything_is_loaded(tmp_path):
    c, f = tmp_path / "c.jsonl", tmp_path / "r.jsonl"
    c.write_text('{"id": "yn", "states": [{"edges": [[1, 0]], "accept": true}]}\n')
    f.write_text('{"tokens": [1, 2], "constraint": "yn"}\n{"tokens": [3], "constraint": "other"}\n')
    with pytest.raises(SystemExit, match=r"--constraints: request line 2: unknown constraint 'other'"):
        G.main(_args("--synthetic", "tiny-test", "--batch_size", "4", "--requests", str(f), "--constraints", str(c)))
    with pytest.raises(SystemExit, match=r"--requests: request line 1: unknown constraint 'yn'"):
        G.main(_args("--synthetic", "tiny-test", "--batch_size", "4", "--requests", str(f)))
    c.write_text('{"id": "yn", "states": []}\n')
    with pytest.raises(SystemExit, match=r"--constraints: constraint line 1: an automaton needs at least one state"):
        G.main(_args("--synthetic", "tiny-test", "--batch_size", "4", "--requests", str(f), "--constraints", str(c)))


# ---- the ABI and the build --------------------------------------------------------------------------------------------------------------
def test_constrain_entry_point_is_declared_listed_and_registered():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    assert "teal_constrain_logits" in _lib.EXPORTS and re.search(r"\bteal_constrain_logits\(", hdr)
    assert "teal_constrain_logits" in _lib.OPTIONAL_WITH_OVERRIDE and "teal_constrain.hip" in _lib.SOURCES
    assert os.path.exists(os.path.join(_lib.CSRC, "teal_constrain.hip"))
    assert int(re.search(r"#define TEAL_CONSTRAIN_VIOLATION \(1 << (\d+)\)", hdr).group(1)) == 30 and CN.VIOLATION == R.VIOLATION == 1 << 30
    assert int(re.search(r"#define TEAL_CONSTRAIN_STATE_MASK (0x[0-9A-F]+)", hdr).group(1), 16) == CN.STATE_MASK == R.STATE_MASK


def test_constrain_kernel_does_not_spill_to_scratch(tmp_path):
    res = _resources(tmp_path, "teal_constrain.hip")
    assert len(res) == 1 and "constrain_logits_kernel" in next(iter(res)), sorted(res)
    assert all(v == (0, 0) for v in res.values()), res


# ---- SamplerFeatures --------------------------------------------------------------------------------------------------------------------
class _Host(EF.SamplerFeatures):
    def __init__(self):
        self._feature_rows = 2
        self.cfg = type("Cfg", (), {"vocab_size": 16})()
        self.dtype, self.code = torch.float16, 0
        self.history = torch.zeros(2, 5, dtype=torch.int32)
        self.rng_state = torch.zeros(2, 2, dtype=torch.int64)
        self.tok_buf, self.pos_buf = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
        self._graph = "captured"
        self.log = []

    def _sample_row(self, row, logits, temperature, top_k, feed, st):
        self.log.append(("hook", (row, logits.data_ptr())))

    def _eos_words(self, row0):
        return 0xE05000 + 4 * row0


class _Rec:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return lambda *a: self._log.append((name, a)) or 0


def test_off_state_key_and_loop_state_are_unchanged_and_the_chain_gains_one_launch(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)
    h = _Host()
    assert h._con is None and h._feature_key() == (None, False) and h._feature_loop_state() == []
    with pytest.raises(RuntimeError) as e:
        h._constraints()
    assert str(e.value) == "constraints are off (set_constraints)"
    with pytest.raises(NotImplementedError, match="_Host has no constrained decoding.*only SlotDecodeEngine"):
        h.set_constraints(True)  # DecodeEngine's and BatchedDecodeEngine's setter: they have no admission and no EOS word
    h.set_constraints(False)
    assert h._con is None and h._graph == "captured"
    logits = torch.zeros(2, 16, dtype=torch.float16)
    h._draw(logits, 16, 2, 0.7, 40, h.rng_state, h.tok_buf, h.pos_buf, h.history, True, st=77)
    assert h.log == [("hook", (0, logits[0].data_ptr())), ("hook", (1, logits[1].data_ptr()))]  # off: exactly the launches of before

    h._con = c = CN.Constraints(2, 16, torch.float16, 5, "cpu", capacity_words=64)
    c.L = _Rec(h.log)
    assert h._feature_key() == (None, False, "constraints") and [id(t) for t in h._feature_loop_state()] == [id(c.trace)]
    del h.log[:]
    h._active = 0xAC7000
    h._draw(logits, 16, 2, 0.7, 40, h.rng_state, h.tok_buf, h.pos_buf, h.history, True, st=77)
    assert h.log == [("teal_constrain_logits", (logits.data_ptr(), 16, 16, 0, 2, h.tok_buf.data_ptr(), h.rng_state.data_ptr(), 0xE05000,
                                                c.table.data_ptr(), c.arena.data_ptr(), 64, c.trace.data_ptr(), 5, c.con.data_ptr(), 16,
                                                0xAC7000, 0, 77)),
                     ("hook", (0, c.con[0].data_ptr())), ("hook", (1, c.con[1].data_ptr()))]
    # with the processors on the chain is adjust -> constrain -> sample, and an admission's one row is handed on as it stands
    h.set_logit_processors(True)
    h._proc.L = _Rec(h.log)
    del h.log[:]
    row = torch.zeros(16, dtype=torch.float16)
    h._draw(row, 0, 1, 0.7, 40, h.rng_state[1], h.tok_buf[1:], h.pos_buf[1:], h.history[1], False, row0=1, st=77)
    (n0, a0), (n1, a1), (n2, a2) = h.log
    assert (n0, n1, n2) == ("teal_logit_adjust", "teal_constrain_logits", "hook")
    assert a0[0] == row.data_ptr() and a0[10] == h._proc.adj[1].data_ptr()
    assert a1[0] == h._proc.adj[1].data_ptr() and a1[1] == 0 and a1[4] == 1 and a1[7] == 0xE05004 and a1[8] == c.table[1].data_ptr()
    assert a1[11] == c.trace[1].data_ptr() and a1[13] == c.con[1].data_ptr() and a1[15:] == (0xAC7000, 1, 77)
    assert a2 == (1, c.con[1].data_ptr())
