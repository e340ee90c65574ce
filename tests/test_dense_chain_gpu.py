"""GPU: which entry points the three dense slab-chain passes call, in order — the prompt pass (PrefillEngine), the verify / suffix
pass (VerifyPass.run) and the two admissions of a SlotDecodeEngine that run them at a slot's cache base (plain: the prompt pass;
on a prefix: the verify pass) — against a literal table.  The batched and slot STEP's table is in test_draw_chain_gpu.py.
`tiny-test` (2 layers, dim 256, head_dim 64, intermediate 512, vocab 512), fp16 and one bf16 case.  The recorder sits on the
pass's own library handle, so a launch that moved, doubled or dropped shows; for the slot cases it also keeps the attention
calls' arguments: the K / V pointers must be the slot's base addresses."""
import pytest
import torch

from test_continuous_gpu import _model
from test_logit_engine_gpu import KW, _Count
from teal_amd.gpt_fast.batched import SlotDecodeEngine
from teal_amd.gpt_fast.prefill import PrefillEngine
from teal_amd.gpt_fast.speculative import VerifyPass

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_LAYER, B, MAX_SEQ = 2, 3, 64
GEMM, RESID = "teal_prefill_gemm", "teal_prefill_resid_norm"


def _chain(attention):
    """the embedding rows; per layer qkv, the pass's attention, wo, resid, gate|up, down, resid"""
    return [RESID] + [GEMM, attention, GEMM, RESID, GEMM, GEMM, RESID] * N_LAYER


# ... and each pass's own tail: the lm_head GEMV of the last token / the lm_head GEMM of every row (/ the last row rounded)
PROMPT = _chain("teal_prefill_attention") + ["teal_sparse_qkv_gemv_ld"]
VERIFY = _chain("teal_verify_attention") + [GEMM]
SUFFIX = VERIFY + ["teal_batched_round_rows"]
KV_ARGS = {"teal_prefill_attention": (3, 4), "teal_verify_attention": (4, 5)}  # where the K / V cache pointers stand


class _CountAttention(_Count):
    """_Count that also keeps (k_cache, v_cache) of every attention call"""

    def __init__(self, L, calls, kv):
        super().__init__(L, calls)
        self._kv = kv

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name not in KV_ARGS:
            return call

        def keep(*a):
            self._kv.append(tuple(a[i] for i in KV_ARGS[name]))
            return call(*a)
        return keep


def _calls(obj, fn):
    calls, kv = [], []
    lib = obj.L
    obj.L = _CountAttention(lib, calls, kv)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        obj.L = lib
    return calls, kv


def _tokens(n, seed=5):
    return torch.randint(0, 512, (n,), device=DEV, dtype=torch.int32, generator=torch.Generator(device=DEV).manual_seed(seed))


@pytest.mark.parametrize("dt,T", [(torch.float16, 2), (torch.float16, 8), (torch.float16, 9), (torch.float16, 16), (torch.bfloat16, 9)])
def test_prompt_pass(dt, T):
    m, _ = _model("tiny-test", dt, 1, MAX_SEQ)
    eng = PrefillEngine(m)
    calls, _ = _calls(eng, lambda: eng(_tokens(T)))
    assert calls == PROMPT


@pytest.mark.parametrize("T", [2, 9])
def test_verify_pass(T):
    m, _ = _model("tiny-test", torch.float16, 1, MAX_SEQ)
    eng = VerifyPass(m)
    pos = torch.tensor([5], dtype=torch.int32, device=DEV)
    calls, _ = _calls(eng, lambda: eng.run(_tokens(T), pos, T))
    assert calls == VERIFY


def _slot_bases(m, s):
    return [(l.attention.kv_cache.k_cache[s].data_ptr(), l.attention.kv_cache.v_cache[s].data_ptr()) for l in m.layers]


def test_slot_admission_runs_the_prompt_pass_at_the_slots_caches():
    m, ths = _model("tiny-test", torch.float16, B, MAX_SEQ)
    eng = SlotDecodeEngine(m, ths, B)
    eng.admit(0, [5, 9, 300, 9, 17], 20, None, 21, **KW)  # (the slot prompt pass is made at the first admission)
    calls, kv = _calls(eng._prefill, lambda: eng.admit(2, [7, 450, 2], 20, None, 23, **KW))
    assert calls == PROMPT and eng.admit_paths == {"hip": 2, "module": 0}
    assert kv == _slot_bases(m, 2)


def test_slot_admission_on_a_prefix_runs_the_verify_pass_at_the_slots_caches():
    m, ths = _model("tiny-test", torch.float16, B, MAX_SEQ)
    eng = SlotDecodeEngine(m, ths, B)
    eng.register_prefix("p", [11, 4, 205, 4, 90])
    eng.admit(0, [5, 9], 20, None, 21, prefix="p", **KW)  # (the slot verify pass is made at the first suffix)
    calls, kv = _calls(eng._verify, lambda: eng.admit(2, [7, 450, 2], 20, None, 23, prefix="p", **KW))
    assert calls == SUFFIX and eng.prefix_paths == {"hip": 2, "module": 0}
    assert kv == _slot_bases(m, 2)
