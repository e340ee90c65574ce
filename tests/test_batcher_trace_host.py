"""CPU: ContinuousBatcher makes the engine calls its parent made — the same methods in the same order with the same arguments —
and returns the same results, for every workload of tests/batcher_trace.py.

tests/golden/batcher_trace_parent.json is the record scripts/record_batcher_trace.py took of the commit before each per-request
feature (prefix, logprobs, logit processors, sampling, stop conditions, constraints, sparsity) became one object in continuous.py:
plain runs, every feature switched on by one request or by a batcher default alone, the cases that must NOT switch a feature on,
all seven mixed over two run() calls of one batcher, and every refusal that is raised before anything runs.
"""
import json
import os

import pytest

import batcher_trace as T

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batcher_trace_parent.json")) as _f:
    PARENT = json.load(_f)["workloads"]

SWITCHES = ("set_logprobs", "set_logit_processors", "set_sampling_params", "set_stop_conditions", "set_constraints", "set_slot_sparsity")


def test_the_record_covers_every_workload():
    assert sorted(PARENT) == sorted(T.workloads())


@pytest.mark.parametrize("name", sorted(T.workloads()))
def test_batcher_reproduces_the_parents_trace(name):
    got, want = T.record(name), PARENT[name]
    assert got.get("error") == want.get("error")
    assert len(got["trace"]) == len(want["trace"])
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"call {i}"
    assert got.get("results") == want.get("results")


def test_the_record_holds_what_the_workloads_are_for():
    """the record itself: a refusal left no call behind; a feature that must stay off issued no switch; all seven mixed switch each
    engine feature once, in the first of the two runs, and the two orders of one set of choices share one registered image"""
    for name, w in PARENT.items():
        called = [c[0] for c in w["trace"]]
        if name.startswith("refusal/"):
            assert w["trace"] == [] and w["error"][0] == "ValueError" and w["error"][1], name
        if name.startswith("plain/") or name.split("/")[-1] in ("identity", "plain", "none", "unnamed", "the_runs_level"):
            assert not [c for c in called if c in SWITCHES], name
            assert all(len(c[1]) == 7 and c[2] == {} for c in w["trace"] if c[0] == "admit"), name
    every = PARENT["everything"]
    called = [c[0] for c in every["trace"]]
    assert [called.count(s) for s in SWITCHES] == [1] * len(SWITCHES)
    second_run = called.index("union_kept") + 1   # (a run's last call)
    assert not [c for c in called[second_run:] if c in SWITCHES] and called[second_run:].count("admit") == 24
    assert len(every["results"]) == 2 and every["results"][0]["tokens"] == every["results"][1]["tokens"]
    registered = [c[1][0] for c in every["trace"] if c[0] == "register_constraint"]
    assert sorted(registered) == sorted(set(registered)) and sum(n.startswith("choices:") for n in registered) == 1
    assert [c[1][0] for c in every["trace"] if c[0] == "register_prefix"] == ["sys", "unused"]
