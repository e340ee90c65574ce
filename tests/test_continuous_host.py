"""CPU: continuous batching (teal_batched.hip's slot entry points, teal_amd/gpt_fast/continuous.py) — what needs no GPU.

  * the slot kernels (teal_batched.hip, and the slot-predicated sampler in teal_sampler.hip) build for gfx950 with no scratch
    and no VGPR spills, and the new entry points are exported and declared;
  * ContinuousBatcher against a fake engine that restates the device rule (retire on budget / EOS, per-request draws):
    FIFO admission, slot reuse, min(budget, up to EOS) tokens per request, refill="all", refusals;
  * JSON Lines parsing and generate.py --requests' refusals.
"""
import os
import re
import subprocess

import pytest

from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_BUDGET, SLOT_EOS, SLOT_FINISH, SLOT_PRODUCED, SLOT_STEP, SLOT_WORDS
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request, cache_rows, parse_requests

NEW = ("teal_batched_sparse_gemm_slots", "teal_batched_decode_attention_slots", "teal_batched_retire", "teal_sample_topk_slot")


def _resources(tmp_path, name):
    src = os.path.join(_lib.CSRC, name)
    extra = ["-mllvm", f"-amdgpu-kernarg-preload-count={_lib.PRELOAD[name]}"] if name in _lib.PRELOAD else []
    cmd = [_lib._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", f"-I{_lib.INCLUDE}", f"-I{_lib.CSRC}",
           *_lib.NO_PACKED_FP32, _lib.FP_CONTRACT, *extra, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    assert len(scratch) == len(names) == len(spills), (len(names), len(scratch), len(spills))
    return dict(zip(names, zip(scratch, spills)))


def test_slot_kernels_do_not_spill_to_scratch(tmp_path):
    res = _resources(tmp_path, "teal_batched.hip")
    slot = {n: v for n, v in res.items() if "ELb1EEEv" in n or "retire" in n}  # the SLOTS = true instantiations and the retire launch
    assert len(slot) >= 24 + 4 + 2 + 1, sorted(slot)
    assert all(v == (0, 0) for v in slot.values()), {n: v for n, v in slot.items() if v != (0, 0)}
    res = _resources(tmp_path, "teal_sampler.hip")
    samp = {n: v for n, v in res.items() if "slot_kernel" in n}
    assert len(samp) == 8, sorted(samp)
    # (the 16-vectors-per-thread window sampler — Llama-3's vocabulary — spills in its plain form already, 1024 threads leave it
    #  128 VGPRs; its slot form is the same kernel behind one early exit and may spill no more than a few registers beyond it)
    for n, v in samp.items():
        if "window_slot_kernelILb" in n and "ELi16E" in n:
            plain = [pv for pn, pv in res.items() if "25sample_topk_window_kernel" in pn and "ELi16E" in pn and pn[33:37] == n[38:42]]
            assert plain and v[1] <= plain[0][1] + 8, (n, v, plain)
        else:
            assert v == (0, 0), (n, v)


def test_slot_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\(", hdr), name
    offs = {m: int(v) for m, v in re.findall(r"#define TEAL_SLOT_(\w+) (\d+)", hdr)}
    assert offs == {"ACTIVE": SLOT_ACTIVE, "STEP": SLOT_STEP, "BUDGET": SLOT_BUDGET, "PRODUCED": SLOT_PRODUCED, "EOS": SLOT_EOS,
                    "FINISH": SLOT_FINISH, "WORDS": SLOT_WORDS}


# ---- the scheduler against a fake engine ------------------------------------------------------------------------------------
def _draw(seed, i, vocab=50):
    return (seed * 7919 + i * 104729 + (seed * i) % 13) % vocab


class FakeEngine:
    """the device rule on the host: admit draws token 0 and retires as teal_batched_retire would; a step draws token i of each
    active slot's stream, then retires"""

    def __init__(self, B=4, max_seq=64):
        self.B, self.max_seq = B, max_seq
        self.state = [0] * SLOT_WORDS
        for b in range(8):
            self.state[SLOT_EOS + b] = self.state[SLOT_FINISH + b] = -1
        self.hist = [[] for _ in range(B)]
        self.seed, self.pos = [0] * B, [0] * B
        self.log, self.reads = [], 0

    def _retire(self, mask, count_step):
        st = self.state
        for b in range(self.B):
            if (mask >> b) & 1 and (st[SLOT_ACTIVE] >> b) & 1:
                st[SLOT_BUDGET + b] -= 1
                st[SLOT_PRODUCED + b] += 1
                if st[SLOT_BUDGET + b] <= 0 or self.hist[b][-1] == st[SLOT_EOS + b] or self.pos[b] >= self.max_seq:
                    st[SLOT_ACTIVE] &= ~(1 << b)
                    st[SLOT_FINISH + b] = st[SLOT_STEP]
        if count_step:
            st[SLOT_STEP] += 1

    def admit(self, slot, tokens, budget, eos_id, seed, temperature, top_k):
        assert not (self.state[SLOT_ACTIVE] >> slot) & 1, "admitted into a busy slot"
        self.log.append((slot, seed, self.state[SLOT_STEP]))
        self.seed[slot], self.pos[slot] = seed, len(tokens)
        self.state[SLOT_BUDGET + slot], self.state[SLOT_PRODUCED + slot] = budget, 0
        self.state[SLOT_EOS + slot] = -1 if eos_id is None else eos_id
        self.state[SLOT_ACTIVE] |= 1 << slot
        self.hist[slot] = [_draw(seed, 0)]
        self._retire(1 << slot, False)

    def run_steps(self, k, temperature, top_k, use_graph):
        for _ in range(k):
            for b in range(self.B):
                if (self.state[SLOT_ACTIVE] >> b) & 1:
                    self.hist[b].append(_draw(self.seed[b], len(self.hist[b])))
                    self.pos[b] += 1
            self._retire((1 << self.B) - 1, True)

    def read_state(self):
        self.reads += 1
        return list(self.state)

    def read_history(self, slot, n):
        return self.hist[slot][:n]

    def union_kept(self):
        return {}


def _expected(req, r, seed=1234):
    toks = [_draw(seed + r, i) for i in range(req.max_new_tokens)]
    if req.eos_id is not None and req.eos_id in toks:
        toks = toks[:toks.index(req.eos_id) + 1]
    return toks


REQS = [Request([1, 2, 3], n) for n in (5, 17, 3, 9, 1, 12, 7, 2, 20, 4)]


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("refill", ["free", "all"])
def test_every_request_gets_its_budget_from_its_own_stream(K, refill):
    eng = FakeEngine()
    res = ContinuousBatcher(eng, sync_every=K, refill=refill).run(REQS)
    assert res["tokens"] == [_expected(q, r) for r, q in enumerate(REQS)]
    assert res["admissions"] == len(REQS) and res["useful_tokens"] == sum(q.max_new_tokens for q in REQS)
    assert 0 < res["mean_active_slots"] <= eng.B


def test_admission_is_fifo_and_slots_are_reused():
    eng = FakeEngine()
    ContinuousBatcher(eng, sync_every=2).run(REQS)
    seeds = [s for _, s, _ in eng.log]
    assert seeds == [1234 + r for r in range(len(REQS))]  # FIFO
    slots = [s for s, _, _ in eng.log]
    assert slots[:4] == [0, 1, 2, 3] and len(set(slots)) == 4  # the 10 requests reuse the 4 slots
    # request 4 (budget 1) ends at admission; request 2 (budget 3) frees its slot after the first burst: both refilled early
    assert [step for _, _, step in eng.log][4] == 2


def test_refill_all_waits_for_every_slot():
    eng = FakeEngine()
    ContinuousBatcher(eng, sync_every=1, refill="all").run(REQS)
    steps = [step for _, _, step in eng.log]
    for g in range(0, len(REQS), 4):  # groups of B admitted together, the next only once the group's longest is done
        assert len(set(steps[g:g + 4])) == 1
    assert steps[4] == max(q.max_new_tokens for q in REQS[:4]) - 1  # (its first token comes from admission)


def test_continuous_beats_static_batching_in_steps():
    a = ContinuousBatcher(FakeEngine(), sync_every=1, refill="free").run(REQS)
    b = ContinuousBatcher(FakeEngine(), sync_every=1, refill="all").run(REQS)
    assert a["tokens"] == b["tokens"] and a["steps"] < b["steps"] and a["mean_active_slots"] > b["mean_active_slots"]


def test_eos_cuts_right_after_its_first_occurrence():
    eos = _draw(1234 + 1, 4)  # token 4 of request 1
    reqs = [Request(q.tokens, q.max_new_tokens, eos) for q in REQS]
    res = ContinuousBatcher(FakeEngine(), sync_every=3).run(reqs)
    for r, (q, got) in enumerate(zip(reqs, res["tokens"])):
        full = _expected(Request(q.tokens, q.max_new_tokens), r)
        assert got == _expected(q, r) and got == full[:len(got)]
        assert len(got) == (full.index(eos) + 1 if eos in full else q.max_new_tokens)
    assert len(res["tokens"][1]) == 5


def test_oversize_requests_are_refused_before_anything_runs():
    eng = FakeEngine(max_seq=16)
    with pytest.raises(ValueError, match="do not fit"):
        ContinuousBatcher(eng).run([Request([1] * 4, 8), Request([1] * 10, 7)])
    assert eng.log == [] and eng.reads == 0
    with pytest.raises(ValueError, match="block_size"):
        cache_rows([Request([1] * 100, 40)], 128)
    assert cache_rows([Request([1] * 5, 10), Request([1] * 30, 3)], 128) == 33


def test_parse_requests():
    lines = ['{"tokens": [1, 2, 3]}', "", '{"tokens": [4], "max_new_tokens": 7}']
    rs = parse_requests(lines, 20, eos_id=2)
    assert [(r.tokens, r.max_new_tokens, r.eos_id) for r in rs] == [([1, 2, 3], 20, 2), ([4], 7, 2)]

    class Tok:
        def bos_id(self):
            return 1

        def encode(self, s):
            return [ord(c) for c in s]
    assert parse_requests(['{"prompt": "hi"}'], 5, Tok())[0].tokens == [1, ord("h"), ord("i")]
    for bad, msg in [('{"prompt": "hi"}', "tokenizer"), ('{"tokens": []}', "non-empty"), ('{"tokens": [1], "prompt": "x"}', "exactly one"),
                     ('{"tokens": [1], "max_new_tokens": 0}', "positive"), ("not json", "not JSON"), ('{"tokens": [-1]}', "token ids"),
                     ('{"tokens": [1, true]}', "token ids")]:
        with pytest.raises(ValueError, match=msg):
            parse_requests([bad], 5)
    with pytest.raises(ValueError, match="no requests"):
        parse_requests(["", " "], 5)


def _args(*extra):
    return G.build_parser().parse_args(["--device", "cuda", *extra])


@pytest.mark.parametrize("extra,msg", [
    (("--synthetic", "tiny-test", "--batch_size", "4", "--self_speculate"), "speculative"),
    (("--synthetic", "tiny-test", "--batch_size", "9"), "1..8"),
    (("--synthetic", "tiny-test", "--interactive"), "interactive"),
    (("--checkpoint_path", "ck/Llama-2-7b-int8/model.pth", "--hist_path", "h"), "16-bit"),
    (("--checkpoint_path", "ck/Llama-2-7b-int4/model.pth", "--hist_path", "h", "--batch_size", "4"), "16-bit"),
    (("--synthetic", "tiny-test", "--batch_size", "4", "--compile", "--no_engine"), "no_engine"),
    (("--synthetic", "tiny-test", "--batch_size", "4", "--no_fused_decode"), "no_fused_decode"),
    (("--synthetic", "tiny-test", "--batch_size", "4", "--dense"), "thresholds"),
    (("--synthetic", "tiny-test", "--batch_size", "4", "--sync_every", "0"), "sync_every"),
])
def test_generate_requests_refusals(extra, msg, tmp_path):
    f = tmp_path / "r.jsonl"
    f.write_text('{"tokens": [1, 2]}\n')
    with pytest.raises(SystemExit, match=msg):
        G.main(_args("--requests", str(f), *extra))


def test_generate_requests_refuses_tensor_parallel(monkeypatch, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor parallelism"):
        G.check_requests_args(_args("--synthetic", "tiny-test", "--requests", str(tmp_path / "r.jsonl")))


def test_requests_flags_default_off():
    a = _args()
    assert a.requests is None and a.eos_id is None and a.sync_every == 8
