"""What ContinuousBatcher asks of its engine, call by call: a recording fake engine and named workloads.  Every call the batcher
makes — method, arguments, keywords — and every result dict are pinned by tests/golden/batcher_trace_parent.json (recorded by
scripts/record_batcher_trace.py on the commit BEFORE the per-request features were gathered into one object each);
tests/test_batcher_trace_host.py holds the batcher to that record, entry for entry.

Nothing here imports more of continuous.py than Request and ContinuousBatcher, so the same file runs on either side of that change.
"""
import json
from types import SimpleNamespace

from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_BUDGET, SLOT_EOS, SLOT_FINISH, SLOT_PRODUCED, SLOT_STEP, SLOT_WORDS
from teal_amd.gpt_fast.constraints import Automaton
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request

VOCAB = 50
TIMINGS = ("wall_s", "admission_s", "admission_share", "useful_tokens_per_sec")  # what a result dict holds of the clock


def _draw(seed, i):
    return (seed * 7919 + i * 104729 + (seed * i) % 13) % VOCAB


def _plain(v):
    """an argument as JSON holds it"""
    if isinstance(v, Automaton):
        return {"automaton": v.to_json()["states"]}
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


class RecordingEngine:
    """The device rule on the host, with every optional method of the batcher's protocol.  Its answers depend on its arguments
    and on nothing else: token i of a request is _draw(seed, i), a slot retires on its budget, its EOS id, the cache end or a
    stop condition, a logprob is a function of the token, and a slot "keeps" 1 - thresholds[0]["q"] of the rows (half of them
    without thresholds).  `log` is every call, in order: [method, args, kwargs]."""

    def __init__(self, B, max_seq=64):
        self.B, self.max_seq, self.cfg = B, max_seq, SimpleNamespace(vocab_size=VOCAB)
        self.state = [0] * SLOT_WORDS
        for b in range(8):
            self.state[SLOT_EOS + b] = self.state[SLOT_FINISH + b] = -1
        self.hist = [[] for _ in range(B)]
        self.seed, self.pos = [0] * B, [0] * B
        self.stops = [{} for _ in range(B)]
        self.finish = [(None, -1)] * B
        self.level, self.ran = [None] * B, [0] * B
        self.top_n = 0
        self.prefixes, self.constraints, self.prefix_paths = {}, {}, {"hip": 0, "module": 0}
        self.log = []

    def _call(self, method, *args, **kw):
        self.log.append([method, _plain(args), _plain(kw)])

    # ---- the device rule ---------------------------------------------------------------------------------------------------
    def _stopped(self, b):
        h, st = self.hist[b], self.stops[b]
        if len(h) < st.get("min_new_tokens", 0):
            return None
        if h[-1] in st.get("stop_token_ids", ()):
            return "stop_token", h[-1]
        for j, q in enumerate(st.get("stop_sequences", ())):
            if h[-len(q):] == list(q):
                return "stop_sequence", j
        if h[-1] == self.state[SLOT_EOS + b]:
            return "stop_token", h[-1]
        return None

    def _retire(self, mask, count_step):
        st = self.state
        for b in range(self.B):
            if (mask >> b) & 1 and (st[SLOT_ACTIVE] >> b) & 1:
                st[SLOT_BUDGET + b] -= 1
                st[SLOT_PRODUCED + b] += 1
                why = self._stopped(b) or (("length", -1) if st[SLOT_BUDGET + b] <= 0 else None) or \
                    (("cache", -1) if self.pos[b] >= self.max_seq else None)
                if why is not None:
                    st[SLOT_ACTIVE] &= ~(1 << b)
                    st[SLOT_FINISH + b] = st[SLOT_STEP]
                    self.finish[b] = why
        if count_step:
            st[SLOT_STEP] += 1

    # ---- the protocol ------------------------------------------------------------------------------------------------------
    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k, **kw):
        self._call("admit", slot, tokens, budget, eos_id, seed, temperature, top_k, **kw)
        assert not (self.state[SLOT_ACTIVE] >> slot) & 1, "admitted into a busy slot"
        P = len(self.prefixes[kw["prefix"]]) if "prefix" in kw else 0
        self.prefix_paths["hip"] += 1 if P else 0
        self.seed[slot], self.pos[slot] = seed, P + len(tokens)
        self.state[SLOT_BUDGET + slot], self.state[SLOT_PRODUCED + slot] = budget, 0
        self.state[SLOT_EOS + slot] = -1 if eos_id is None else eos_id
        self.state[SLOT_ACTIVE] |= 1 << slot
        self.stops[slot] = {k: kw[k] for k in ("stop_token_ids", "stop_sequences", "min_new_tokens") if k in kw}
        self.finish[slot] = (None, -1)
        self.level[slot] = kw["thresholds"][0]["q"] if "thresholds" in kw else 0.5
        self.hist[slot] = [_draw(seed, 0)]
        self._retire(1 << slot, False)

    def run_steps(self, k, temperature, top_k, use_graph):
        self._call("run_steps", k, temperature, top_k, use_graph)
        for _ in range(k):
            self.ran = [(self.state[SLOT_ACTIVE] >> b) & 1 for b in range(self.B)]
            for b in range(self.B):
                if self.ran[b]:
                    self.hist[b].append(_draw(self.seed[b], len(self.hist[b])))
                    self.pos[b] += 1
            self._retire((1 << self.B) - 1, True)

    def read_state(self):
        self._call("read_state")
        return list(self.state)

    def read_history(self, slot, n):
        self._call("read_history", slot, n)
        return self.hist[slot][:n]

    def union_kept(self):
        self._call("union_kept")
        return {"q": 0.5}

    def has_prefix(self, name):
        self._call("has_prefix", name)
        return name in self.prefixes

    def register_prefix(self, name, tokens):
        self._call("register_prefix", name, tokens)
        self.prefixes[name] = list(tokens)

    def set_logprobs(self, n):
        self._call("set_logprobs", n)
        self.top_n = n

    def read_logprobs(self, slot, n):
        self._call("read_logprobs", slot, n)
        h = self.hist[slot][:n]
        return ([-(t % 7) / 8 for t in h], [[(t + j) % VOCAB for j in range(self.top_n)] for t in h],
                [[-(t % 7 + j) / 8 for j in range(self.top_n)] for t in h])

    def set_logit_processors(self, on):
        self._call("set_logit_processors", on)

    def set_sampling_params(self, on):
        self._call("set_sampling_params", on)

    def set_stop_conditions(self, on):
        self._call("set_stop_conditions", on)

    def read_finish(self, slot):
        self._call("read_finish", slot)
        return self.finish[slot]

    def set_constraints(self, on):
        self._call("set_constraints", on)

    def has_constraint(self, name):
        self._call("has_constraint", name)
        return name in self.constraints

    def register_constraint(self, name, automaton):
        self._call("register_constraint", name, automaton)
        self.constraints[name] = automaton

    def set_slot_sparsity(self, on):
        self._call("set_slot_sparsity", on)

    def kept_by_slot(self):
        self._call("kept_by_slot")
        return {p: [(1.0 - self.level[b]) * w if self.ran[b] else 0.0 for b in range(self.B)] for p, w in (("q", 1.0), ("down", 0.5))}


# ---- the workloads: name -> (engine keywords, batcher keywords, one request list per run() of the same batcher) -------------------
BUDGETS = (5, 17, 3, 9, 1, 12, 7, 2, 20, 4)
PF = {"sys": [1, 5, 9, 13], "unused": [2, 4]}
LEVELS = {0.0: [{"q": 0.0}], 0.25: [{"q": 0.25}], 0.75: [{"q": 0.75}]}
YN = {"yn": Automaton.from_allowed([1, 2]), "unused": Automaton.from_allowed([3])}
EOS = _draw(1234 + 1, 4)


def _six(at=None, **fields):
    """six requests; request `at` (None: none of them) carries `fields`"""
    return [Request([1, 2, 3 + r], n, **(fields if r == at else {})) for r, n in enumerate((5, 9, 3, 12, 1, 7))]


def _everything():
    reqs = []
    for r in range(24):
        f = {}
        if r % 4 == 1:
            f["prefix"] = "sys"
        if r % 5 == 2:
            f.update(repetition_penalty=1.25, logit_bias={"7": -2.0})
        if r % 7 == 3:
            f.update(presence_penalty=0.5, frequency_penalty=0.25)
        if r % 6 == 4:
            f.update(temperature=0.5, top_p=0.9)
        if r % 9 == 5:
            f.update(top_k=10, min_p=0.125, seed=77 + r)
        if r % 5 == 0:
            f.update(stop_token_ids=[_draw(1234 + r, 3)], min_new_tokens=2)
        if r % 8 == 6:
            f["stop_sequences"] = [[_draw(1234 + r, 1), _draw(1234 + r, 2)], [49, 48]]
        if r % 6 == 1:
            f["constraint"] = "yn"
        if r == 3:
            f["choices"] = [[4, 5], [6]]
        if r == 15:
            f["choices"] = [[6], [4, 5], [6]]  # the same set in another order, with a repeat: one registered image
        if r % 12 == 8:
            f["allowed_token_ids"] = [9, 3, 3, 27]
        if r % 3 == 2:
            f["sparsity"] = (0.25, 0.5, 0.75, 0.0)[(r // 3) % 4]
        reqs.append(Request([1 + r % 3] * (1 + r % 5), 2 + (r * 7) % 11, EOS if "choices" in f or r % 2 else None, **f))
    return reqs


def workloads():
    w = {}
    for K in (1, 8):
        for refill in ("free", "all"):
            w[f"plain/K{K}/{refill}"] = ({"B": 4}, {"sync_every": K, "refill": refill}, [[Request([1, 2, 3], n) for n in BUDGETS]])
    one = {
        "prefix/request": ({"prefixes": PF}, _six(2, prefix="sys")),
        "prefix/unnamed": ({"prefixes": PF}, _six()),
        "logprobs/0": ({"logprobs": 0}, _six()),
        "logprobs/2": ({"logprobs": 2}, _six()),
        "processors/request": ({}, _six(1, repetition_penalty=1.3, logit_bias={"3": 1.5})),
        "processors/default": ({"frequency_penalty": 0.25}, _six()),
        "processors/identity": ({}, _six(1, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias={})),
        "sampling/request": ({}, _six(3, top_p=0.9)),
        "sampling/temperature": ({}, _six(3, temperature=0.5, seed=99)),
        "sampling/default": ({"min_p": 0.0625}, _six()),
        "sampling/plain": ({"temperature": 0.7, "top_k": 40}, _six(3, temperature=0.7, top_k=40, top_p=1.0, min_p=0.0)),
        "stops/request": ({}, _six(1, stop_token_ids=[_draw(1235, 3)], stop_sequences=[[_draw(1235, 1), _draw(1235, 2)]])),
        "stops/default": ({"stop_token_ids": (_draw(1237, 4),), "min_new_tokens": 2}, _six()),
        "stops/finish_reason": ({"finish_reason": True}, _six()),
        "stops/none": ({"finish_reason": False}, _six(1, stop_token_ids=[], stop_sequences=[], min_new_tokens=0)),
        "constraints/request": ({"constraints": YN}, _six(3, constraint="yn")),
        "constraints/choices": ({}, [Request([1, 2, 3 + r], n, EOS, **({"choices": [[4, 5], [6]]} if r == 3 else {}))
                                     for r, n in enumerate((5, 9, 3, 12, 1, 7))]),
        "constraints/allowed": ({}, _six(0, allowed_token_ids=[8, 2])),
        "constraints/unnamed": ({"constraints": YN}, _six()),
        "sparsity/request": ({"sparsity": 0.5, "sparsity_levels": LEVELS}, _six(1, sparsity=0.75)),
        "sparsity/unknown_run_level": ({"sparsity_levels": LEVELS}, _six(3, sparsity=0.25)),
        "sparsity/the_runs_level": ({"sparsity": 0.5, "sparsity_levels": LEVELS}, _six(1, sparsity=0.5)),
    }
    for name, (kw, reqs) in one.items():
        w[name] = ({"B": 2}, {"sync_every": 2, **kw}, [reqs])
    every = _everything()
    w["everything"] = ({"B": 3}, {"sync_every": 3, "prefixes": PF, "logprobs": 1, "presence_penalty": 0.125, "constraints": YN,
                                  "sparsity": 0.5, "sparsity_levels": LEVELS, "temperature": 0.8, "top_k": 50}, [every, every])
    nine = {i / 16: [{"q": i / 16}] for i in range(9)}
    refusals = {
        "fit": ({"max_seq": 16}, {}, [Request([1] * 4, 8), Request([1] * 10, 7)]),
        "prefix": ({}, {"prefixes": PF}, [Request([1], 2), Request([1], 2, prefix="nope")]),
        "constraint": ({}, {"constraints": YN}, [Request([1], 2), Request([1], 2, constraint="nope")]),
        "choices_without_eos": ({}, {}, [Request([1], 2, choices=[[4, 5]])]),
        "constraint_temperature": ({}, {"constraints": YN, "temperature": 150.0}, [Request([1], 2, constraint="yn")]),
        "level_without_thresholds": ({}, {"sparsity": 0.5, "sparsity_levels": LEVELS}, [Request([1], 2), Request([1], 2, sparsity=0.3)]),
        "nine_levels": ({}, {"sparsity": 0.75, "sparsity_levels": nine}, [Request([1], 2, sparsity=lv) for lv in nine]),
    }
    for name, (ekw, kw, reqs) in refusals.items():
        w["refusal/" + name] = ({"B": 2, **ekw}, kw, [reqs])
    return w


def record(name):
    """one workload on this tree's batcher: {"trace": [...], "results": [...]} — or, refused, {"trace": [], "error": [type, text]} —
    as JSON holds it"""
    ekw, kw, runs = workloads()[name]
    eng = RecordingEngine(**ekw)
    batcher = ContinuousBatcher(eng, **kw)
    out = {"results": []}
    try:
        for reqs in runs:
            res = batcher.run(reqs)
            out["results"].append({k: v for k, v in res.items() if k not in TIMINGS})
    except (ValueError, RuntimeError) as e:
        out = {"error": [type(e).__name__, str(e)]}
    out["trace"] = eng.log
    return json.loads(json.dumps(out))
