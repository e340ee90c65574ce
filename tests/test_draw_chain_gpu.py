"""GPU: which entry points the fused engines call, in order, for one eager decode step, for DecodeEngine.sample_first and for one
SlotDecodeEngine.admit, under every sampler-side feature — against a literal table.  `tiny-test` (2 layers, dim 256, vocab 512),
fp16; DecodeEngine, BatchedDecodeEngine at B = 3 and SlotDecodeEngine at B = 3 with slots 0 and 2 admitted.  The recorder sits on
the engine's library handle and on every feature object's, so a launch that went round them, moved, doubled or dropped shows."""
import pytest
import torch

from test_logit_engine_gpu import KW, _Count, _model
from teal_amd.gpt_fast.batched import BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.engine import DecodeEngine

pytestmark = pytest.mark.gpu
N_LAYER, B = 2, 3

# the forward pass of one step
GEMV, GEMM, RESID = "teal_fused_gemv", "teal_batched_sparse_gemm", "teal_prefill_resid_norm"
FORWARD = {
    # per layer qkv (RoPE and the cache rows in its epilogue), split attention (merged by wo), wo, gate|up, down; then the lm_head
    "decode": [GEMV, "teal_decode_attention_split_roped", GEMV, GEMV, GEMV] * N_LAYER + [GEMV],
    # embedding rows; per layer qkv, attention, wo, resid, gate|up, down, resid; the lm_head and its rounding
    "batched": [RESID] + [GEMM, "teal_batched_decode_attention", GEMM, RESID, GEMM, GEMM, RESID] * N_LAYER + [GEMM, "teal_batched_round_rows"],
    "slot": [RESID] + [GEMM + "_slots", "teal_batched_decode_attention_slots", GEMM + "_slots", RESID, GEMM + "_slots", GEMM + "_slots", RESID] * N_LAYER
            + [GEMM + "_slots", "teal_batched_round_rows"],
}
TOPK = {"decode": "teal_sample_topk_ws", "batched": "teal_sample_topk_ws", "slot": "teal_sample_topk_slot"}
ADJUST, ROWS, LOGPROBS = "teal_logit_adjust", "teal_sample_rows", "teal_token_logprobs"
RETIRE, RETIRE_STOPS = "teal_batched_retire", "teal_batched_retire_stops"


def _draw(kind, setting, rows):
    """the launches that draw `rows` sequences' tokens: processors in front, one sampling launch or a fused sampler per row,
    logprobs behind"""
    return {"off": [TOPK[kind]] * rows,
            "logprobs": [TOPK[kind]] * rows + [LOGPROBS],
            "processors": [ADJUST] + [TOPK[kind]] * rows,
            "sampling": [ROWS],
            "all": [ADJUST, ROWS, LOGPROBS],
            "all+stops": [ADJUST, ROWS, LOGPROBS]}[setting]


def _switch_on(eng, setting):
    if setting == "all+stops":
        eng.set_stop_conditions(True)
    if setting in ("logprobs", "all", "all+stops"):
        eng.set_logprobs(2)
    if setting in ("processors", "all", "all+stops"):
        eng.set_logit_processors(True)
    if setting in ("sampling", "all", "all+stops"):
        eng.set_sampling_params(True)


def _calls(eng, fn):
    calls = []
    held = [(o, o.L) for o in (eng, eng._lp, eng._proc, eng._samp, getattr(eng, "_stops", None)) if o is not None]
    for o, lib in held:
        o.L = _Count(lib, calls)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for o, lib in held:
            o.L = lib
    return calls


SETTINGS = ["off", "logprobs", "processors", "sampling", "all"]


@pytest.mark.parametrize("setting", SETTINGS)
def test_decode_engine_step_and_first_draw(setting):
    m, ths = _model("tiny-test", None, 1)
    eng = DecodeEngine(m, ths)
    _switch_on(eng, setting)
    row = (torch.randn(m.config.vocab_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 3).half()
    assert _calls(eng, lambda: eng.sample_first(row, **KW)) == _draw("decode", setting, 1)
    assert _calls(eng, lambda: eng._self_step(**KW)) == FORWARD["decode"] + _draw("decode", setting, 1)


@pytest.mark.parametrize("setting", SETTINGS)
def test_batched_engine_step(setting):
    m, ths = _model("tiny-test", None, B)
    eng = BatchedDecodeEngine(m, ths, B)
    _switch_on(eng, setting)
    assert _calls(eng, lambda: eng._self_step(**KW)) == FORWARD["batched"] + _draw("batched", setting, B)


@pytest.mark.parametrize("setting", SETTINGS + ["all+stops"])
def test_slot_engine_admission_and_step(setting):
    m, ths = _model("tiny-test", None, B)
    eng = SlotDecodeEngine(m, ths, B)
    _switch_on(eng, setting)
    retire = [RETIRE_STOPS if setting == "all+stops" else RETIRE]
    eng.admit(0, [5, 9, 300, 9, 17], 20, None, 21, **KW)
    # (the prompt pass runs through its own engine's handle: an admission's own launches are its first draw and the retire rule)
    assert _calls(eng, lambda: eng.admit(2, [7, 450, 2], 20, None, 23, **KW)) == _draw("slot", setting, 1) + retire
    assert eng.read_state()[0] == 0b101
    # a step launches for every slot, the free one included: the device predicates them
    assert _calls(eng, lambda: eng._self_step(**KW)) == FORWARD["slot"] + _draw("slot", setting, B) + retire
