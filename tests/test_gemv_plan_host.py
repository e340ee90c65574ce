"""CPU: the GEMV launch plan against the record of the commit before it was gathered in one place.

tests/golden/gemv_plan_parent.json holds, for every case of tests/gemv_plan_cases.py, what a real launch on an MI355X returned,
reported in *nslabs_out and described (scripts/record_gemv_plan.py, run against a build of that commit).  The host-only query
teal_fused_gemv_plan runs the launch's own plan without a device, so here every teal_fused_gemv case must come out as recorded —
code, slab count and description byte for byte — from made-up pointer values.  (The legacy entry points have no query: their
cases are held to the record by the real launches of tests/test_gemv_plan_gpu.py.)"""
import ctypes
import json
import os
import re

import pytest

import gemv_plan_cases as C
from teal_amd import _lib

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_plan_parent.json")) as _f:
    RECORD = json.load(_f)
NUM_CU = RECORD["num_cu"]


def _mismatches(L, cases):
    bad = []
    for c in cases:
        got = list(C.call_plan(L, c, NUM_CU))
        if got != RECORD["fused"][c["id"]]:
            bad.append((c["id"], got, RECORD["fused"][c["id"]]))
    return bad


def test_the_table_is_the_recorded_one():
    assert sorted(c["id"] for c in C.FUSED) == sorted(RECORD["fused"])
    assert sorted(c["id"] for c in C.LEGACY) == sorted(RECORD["legacy"])
    assert NUM_CU == 256 and RECORD["commit"]


def test_the_plan_is_the_parents_case_by_case():
    cases = [c for c in C.FUSED if not C.is_diag(c)]
    assert len(cases) > 250
    bad = _mismatches(_lib.load(), cases)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ (id, plan, record): {bad[:8]}"


def test_the_plan_honours_the_diagnostics_switches_as_the_parents_launch_did():
    D = _lib.load_diag()
    cases = [c for c in C.FUSED if C.is_diag(c)]
    bad, last = [], D.teal_last_launch_desc()
    try:
        for c in cases:
            C.set_switches(D, c["switches"])
            bad += _mismatches(D, [c])
    finally:
        C.set_switches(D, None)
    assert len(cases) > 50 and not bad, f"{len(bad)} of {len(cases)} cases differ (id, plan, record): {bad[:8]}"
    assert D.teal_last_launch_desc() == last  # a query launches nothing: the description of the last LAUNCH stands


def test_the_query_follows_no_pointer_and_needs_only_their_identities():
    """other made-up addresses, the same answers"""
    L = _lib.load()
    other = C.Memory(0x10_0000, 0x5555_0000_0000, 0x20_0000, 0x30_0000)
    for c in C.FUSED[::7]:
        if not C.is_diag(c):
            assert list(C.call_plan(L, c, NUM_CU, other)) == RECORD["fused"][c["id"]], c["id"]


def test_the_querys_own_refusals():
    L = _lib.load()
    c = next(c for c in C.FUSED if c["id"] == "7b.wqkv.slabs")
    gin, gout, _desc = C.materialise(c, C.FAKE)
    ns = ctypes.c_int(-1)
    args = (c["Z"], c["dtype"], 1, C.WS_BYTES, NUM_CU, ctypes.byref(ns))
    assert L.teal_fused_gemv_plan(None, ctypes.byref(gout), *args) == -1
    assert L.teal_fused_gemv_plan(ctypes.byref(gin), None, *args) == -1
    assert L.teal_fused_gemv_plan(ctypes.byref(gin), ctypes.byref(gout), c["Z"], 2, 1, C.WS_BYTES, NUM_CU, ctypes.byref(ns)) == -2
    assert L.teal_fused_gemv_plan(ctypes.byref(gin), ctypes.byref(gout), c["Z"], c["dtype"], 1, C.WS_BYTES, 0, ctypes.byref(ns)) == -1
    assert ns.value == -1
    assert L.teal_fused_gemv_plan(ctypes.byref(gin), ctypes.byref(gout), *args) == 0 and ns.value == RECORD["fused"][c["id"]][1]
    # the CU count is an argument: half the chip plans another launch
    gin, gout, desc = C.materialise(next(c for c in C.FUSED if c["id"] == "7b.wo.plain.ticketed"), C.FAKE)
    assert L.teal_fused_gemv_plan(ctypes.byref(gin), ctypes.byref(gout), 4096, C.BF16, 1, C.WS_BYTES, 128, ctypes.byref(ns)) == 0
    assert ns.value == 2 and desc.value.decode().endswith("grid (64,2) x 1024")


def test_get_config_reports_the_default_geometry():
    """teal_get_config: the plain rounded 16-bit geometry before any output-kind adjustment — what a ROUNDED launch of 16-bit
    weights is described with (without a device the query assumes 256 CUs)"""
    L = _lib.load()
    for cid, lpr, split in (("7b.wqkv.rounded", 8, 1), ("8b.wo.plain.ticketed", 8, 4), ("7b.lm_head", 16, 1), ("8b.lm_head", 64, 1)):
        c = next(c for c in C.FUSED if c["id"] == cid)
        out = (ctypes.c_int * 5)()
        assert L.teal_get_config(c["Z"], sum(c["cols"]), len(c["cols"]), out) == 0
        assert (out[0], out[1], out[2], out[3]) == (lpr, 16, split, 4), (cid, list(out))
        m = re.search(r"grid \((\d+),(\d+)\)|grid (\d+) x", RECORD["fused"][cid][2])
        assert out[4] == (int(m.group(1)) * int(m.group(2)) if m.group(1) else int(m.group(3))), cid


# ---- the table reaches every outcome of the parent: a condition on the record ---------------------------------------------------------
def _descs(prefix=""):
    return [(k, v[2]) for k, v in RECORD["fused"].items() if v[2].startswith(prefix)] + \
           [(k, v[1]) for k, v in RECORD["legacy"].items() if v[1].startswith(prefix)]


def _lean():
    out = []
    for k, d in _descs("gemv_fast_kernel<"):
        bf, mode, pair, lpr, kr, exact, phase, u, w8, rope = d[len("gemv_fast_kernel<"):d.index(">")].split(",")
        gx, gy = re.search(r"grid \((\d+),(\d+)\)", d).groups()
        out.append(dict(id=k, bf=bf, mode=int(mode), pair=pair == "true", lpr=int(lpr), kr=int(kr), exact=exact == "true",
                        w8=w8 == "true", rope=rope == "true", tiles=int(gx), split=int(gy)))
    return out


def _general():
    out = []
    for k, d in _descs("sparse_gemv_kernel<"):
        lpr, waves, u, bf, mode, krt, pair, w8 = d[len("sparse_gemv_kernel<"):d.index(">")].split(",")
        out.append(dict(id=k, lpr=int(lpr), bf=bf, mode=int(mode), krt=int(krt), pair=pair == "true", w8=w8 == "true"))
    return out


def test_the_record_reaches_every_outcome():
    lean, gen, fused, leg = _lean(), _general(), RECORD["fused"], RECORD["legacy"]
    by_id = {c["id"]: c for c in C.FUSED}
    assert {r["mode"] for r in lean} == {0, 1, 2, 3, 4} and {r["kr"] for r in lean} == {1, 4, 8, 16}
    assert {r["exact"] for r in lean if r["mode"] == 1} == {True, False} and {r["lpr"] for r in lean} == {8, 16}
    assert {r["bf"] for r in lean} == {"true", "false"} and {r["bf"] for r in gen} == {"true", "false"}
    assert any(r["pair"] and r["lpr"] == 8 for r in lean) and any(r["w8"] for r in lean)
    assert any(by_id[r["id"]].get("gate_activated") for r in lean if r["id"] in by_id)
    pair30 = next(r for r in lean if r["id"] == "30b.gateup.pair")
    assert pair30["pair"] and pair30["lpr"] == 16 and pair30["tiles"] == 140  # 17920 columns: 128-column tiles
    assert {by_id[r["id"]]["rope_hd"] for r in lean if r["rope"]} == {64, 128}
    # ticketed split-K and the same request without a prepared workspace
    for a, b in (("7b.wo.plain.ticketed", "7b.wo.plain.reduce"), ("7b.down.silu.ticketed", "7b.down.silu.reduce")):
        assert fused[a][2].startswith("gemv_fast_kernel<") and fused[a][1] > 1
        assert fused[b][2].startswith("sparse_gemv_kernel<") and fused[b][1] == fused[a][1]
    # slab sums, the 70B-class slab geometry, the shallow-split one and the tensor-parallel rank-local shapes
    assert fused["slabsum.split1"][:2] == [0, 1] and "grid (192,1)" in fused["slabsum.split1"][2]
    assert fused["7b.wo.masked.slabsum"][:2] == [0, 1] and "grid (64,4)" in fused["7b.wo.masked.slabsum"][2]
    for cid, grid in (("70b.wqkv.slabs", "(80,3)"), ("70b.wo.merge.slabs", "(64,4)"), ("70b.down.silu.slabs", "(64,4)")):
        r = next(r for r in lean if r["id"] == cid)
        assert r["lpr"] == 16 and grid in fused[cid][2], cid
    # tiles x split above the CUs: whole rounds of workgroups (the only cases whose plan depends on that rule: without it
    # 128 x 7 and 128 x 5 slices, more than 8 cached rounds per slice, the general kernel)
    for cid, grid in (("long.65536.slabs.whole_rounds", "(128,8)"), ("long.49152.slabs.whole_rounds", "(128,6)"),
                      ("long.49152.slabsum.whole_rounds", "(128,6)")):
        assert fused[cid][0] == 0 and fused[cid][2].startswith("gemv_fast_kernel<") and "grid " + grid in fused[cid][2], cid
    assert "grid (64,4)" in fused["70b.down.w8.slabs"][2]          # (int8: its own 128-column rule)
    assert "grid (64,2)" in fused["tp2.7b.wo.slabs"][2] and "grid (48,4)" in fused["tp2.8b.wqkv.slabs"][2]
    assert fused["70b.wqkv.rope"][1] == 3 and fused["7b.wqkv.rope"][1] == 0 and fused["diag.split2.wqkv.rope"][1] == 2
    # the general kernel: every tile width, ragged shapes, long vectors, planar slabs, more than 8 slabs
    assert {r["lpr"] for r in gen} == {8, 16, 32, 64} and {r["krt"] for r in gen} == {4, 8, 16}
    assert {r["mode"] for r in gen} == {0, 1, 2, 3, 4} and any(r["pair"] for r in gen) and any(r["w8"] for r in gen)
    assert next(r for r in gen if r["id"] == "yi6b.lm_head")["lpr"] == 32 and next(r for r in gen if r["id"] == "8b.lm_head")["lpr"] == 64
    for cid in ("ragged.z", "ragged.n", "ragged.pair", "long.plain.reduce", "7b.gateup.slabs.planar", "7b.gateup", "ragged.gateup"):
        assert any(r["id"] == cid for r in gen), cid
    assert fused["diag.split16.wo.ticketed"][:2] == [0, 16] and fused["diag.nofast.wqkv.rope"][2].startswith("sparse_gemv_kernel<")
    assert fused["diag.nowl.wo.ticketed"][0] == 0 and fused["diag.lpr32.wo.ticketed"][2].startswith("sparse_gemv_kernel<32,")
    # int4: both kinds, every group size, every producer, tickets / slabs / one slice without a workspace
    i4 = {k: re.match(r"sparse_gemv_int4_kernel<(\w+),(\d),(\d),false> grid \((\d+),(\d+)\)", v[2]).groups()
          for k, v in fused.items() if v[2].startswith("sparse_gemv_int4")}
    assert {g[2] for g in i4.values()} == {"0", "1"} and {g[1] for g in i4.values()} == {"0", "1", "2", "4"}
    assert {by_id[k]["groupsize"] for k in i4} == {32, 64, 128, 256} and {g[0] for g in i4.values()} == {"true", "false"}
    assert i4["7b.i4.wo.nows"][4] == "1" and i4["7b.i4.wo.plainws"][4] == "1" and int(i4["7b.i4.g128.wo.ticketed"][4]) > 1
    # every refusal code of teal_fused_gemv, the int4 path and the legacy entries; CONFIG with and without a description
    assert {v[0] for v in fused.values()} == {0, -1, -2, -3, -4, -5, -8}
    assert {v[0] for k, v in fused.items() if by_id[k]["bits"] == 4} == {0, -1, -3, -5}
    assert {v[0] for v in leg.values()} == {0, -1, -2, -3, -4, -5}
    want = {"refuse.merge.lanes": -3, "175b.pair.44k": -3, "refuse.lds64k": -3, "refuse.ws.small": -5, "refuse.slabs.misaligned": -4,
            "diag.split16.interleave": -8, "refuse.rope.null_table": -1, "refuse.act0.slabs": -1, "refuse.i4.rope": -1,
            "slabsum.ragged.config": -8, "tp2.7b.wo.slabsum.nows": -8}
    assert {k: fused[k][0] for k in want} == want
    assert fused["diag.split16.interleave"][2] and not fused["slabsum.ragged.config"][2]
    assert leg["refuse.sparse.ws.misaligned"][0] == -4 and leg["refuse.gateup.ws.none"][0] == -5
    for fn in ("sparse_gemv", "dense_gemv", "sparse_qkv_gemv", "sparse_qkv_gemv_ld", "sparse_qkv_gemv_i8", "sparse_gateup_silu"):
        assert any(leg[c["id"]][0] == 0 for c in C.LEGACY if c["fn"] == fn), fn


@pytest.mark.parametrize("name", ["teal_fused_gemv_plan"])
def test_the_query_is_declared_and_exported(name):
    header = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "teal_hip.h")).read()
    assert f"int {name}(" in header and name in _lib.EXPORTS and name in _lib.OPTIONAL_WITH_OVERRIDE
    assert hasattr(_lib.load(), name) and hasattr(_lib.load_diag(), name)
