"""Host-side checks of teal_amd/gpt_fast/engine_features.py: the helpers restate, object for object and pointer for pointer, the
expressions they replaced in the engines, and SamplerFeatures keeps the setters' contract (buffers, guards, dropped graph, key)."""
import types

import pytest
import torch

from teal_amd import _lib
from teal_amd.gpt_fast import engine_features as EF
from teal_amd.gpt_fast.batched import BatchedDecodeEngine
from teal_amd.gpt_fast.model import ModelArgs, Transformer
from teal_amd.gpt_fast.prefill import PrefillEngine


def _model(dtype=torch.float16, caches=True):
    torch.manual_seed(0)
    m = Transformer(ModelArgs(block_size=32, vocab_size=64, n_layer=2, n_head=1, dim=64, intermediate_size=128)).to(dtype)
    if caches:
        m.setup_caches(1, 16)
    return m


@pytest.fixture(scope="module")
def model():
    return _model()


def test_linears_are_the_comprehension_they_replace(model):
    lins = [lin for layer in model.layers for lin in (layer.attention.wqkv, layer.attention.wo, layer.feed_forward.w1,
                                                     layer.feed_forward.w3, layer.feed_forward.w2)] + [model.output]
    got = EF.model_linears(model)
    assert len(got) == len(lins) == 11 and all(a is b for a, b in zip(got, lins))
    for layer in model.layers:
        at, ff = layer.attention, layer.feed_forward
        blk = EF.block_linears(layer)
        assert len(blk) == 5 and all(a is b for a, b in zip(blk, (at.wqkv, at.wo, ff.w1, ff.w3, ff.w2)))


def test_pointer_keys_are_the_tuples_they_replace(model):
    m = model
    prefill_key = (m.max_seq_length, m.output.weight.data_ptr(), m.tok_embeddings.weight.data_ptr(), m.freqs_cis.data_ptr()) + tuple(
        p for layer in m.layers for p in (layer.attention.kv_cache.k_cache.data_ptr(), layer.attention.kv_cache.v_cache.data_ptr(),
                                          layer.attention.wqkv.weight.data_ptr(), layer.attention.wo.weight.data_ptr(),
                                          layer.feed_forward.w1.weight.data_ptr(), layer.feed_forward.w2.weight.data_ptr(),
                                          layer.feed_forward.w3.weight.data_ptr()))
    assert EF.pointer_key(m) == prefill_key
    cache_key = (m.max_seq_length,) + tuple(p for layer in m.layers for p in (layer.attention.kv_cache.k_cache.data_ptr(),
                                                                              layer.attention.kv_cache.v_cache.data_ptr()))
    assert EF.pointer_key(m, weights=False) == cache_key
    T = 5
    graphed_key = (T, m.max_seq_length, m.output.weight.data_ptr(), m.tok_embeddings.weight.data_ptr()) + tuple(
        p for layer in m.layers for p in (layer.attention.kv_cache.k_cache.data_ptr(), layer.attention.kv_cache.v_cache.data_ptr(),
                                          layer.attention.wqkv.weight.data_ptr(), layer.attention.wo.weight.data_ptr(),
                                          layer.feed_forward.w1.weight.data_ptr(), layer.feed_forward.w2.weight.data_ptr(),
                                          layer.feed_forward.w3.weight.data_ptr()))
    assert (T,) + EF.pointer_key(m, freqs=False) == graphed_key
    assert len(set(prefill_key[1:])) == len(prefill_key) - 1  # (the pointers are distinct: an order mix-up cannot pass)


class _Host(EF.SamplerFeatures):
    def __init__(self):
        self._feature_rows = 2
        self.cfg = types.SimpleNamespace(vocab_size=16)
        self.dtype = torch.float16
        self.history = torch.zeros(2, 5, dtype=torch.int32)
        self._graph = "captured"


class _Refusing(_Host):
    def _feature_refusal(self, what):
        raise NotImplementedError(f"no {what} here")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)  # (the buffers only keep the handle: nothing is launched here)


def test_sampler_features_setters(no_library):
    h = _Host()
    assert h._feature_key() == (None, False) and h._feature_loop_state() == []
    assert (h.adj_logits, h.lp_state, h.lp_params, h.lp_bias) == (None, None, None, None)
    with pytest.raises(RuntimeError) as e:
        h._logprobs()
    assert str(e.value) == "logprobs are off (set_logprobs)"
    for guarded in (h._processors, lambda: h.set_slot_processors(0, [1, 2])):
        with pytest.raises(RuntimeError) as e:
            guarded()
        assert str(e.value) == "logit processors are off (set_logit_processors)"

    h.set_logprobs(3)
    assert h._graph is None
    lp = h._logprobs()
    assert lp is h._lp and lp.lp.shape == (2, 5) and lp.top_ids.shape == (2, 5, 3) and lp.top_lp.shape == (2, 5, 3)
    assert lp.lp.device == h.history.device
    assert h._feature_key() == (3, False)
    assert [id(t) for t in h._feature_loop_state()] == [id(t) for t in lp.tensors()]

    h._graph = "captured"
    h.set_logit_processors(True)
    assert h._graph is None and h._feature_key() == (3, True)
    pr = h._processors()
    assert pr is h._proc and pr.adj.shape == (2, 16) and pr.adj.dtype == torch.float16
    assert all(a is b for a, b in zip((h.adj_logits, h.lp_state, h.lp_params, h.lp_bias), (pr.adj, pr.state, pr.params, pr.bias)))
    assert [id(t) for t in h._feature_loop_state()] == [id(t) for t in lp.tensors() + pr.loop_tensors()]
    h.set_slot_processors(1, [3, 4], repetition_penalty=1.5, logit_bias={7: -2.0})
    assert pr.params[1].tolist() == [1.5, 0.0, 0.0, 0.0] and float(pr.bias[1, 7]) == -2.0 and pr.params[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert int(pr.state[1, 3]) == -2 ** 31 and int(pr.state[0, 3]) == 0

    h._graph = "captured"
    h.set_logprobs(None)
    assert h._graph is None and h._lp is None and h._feature_key() == (None, True)
    h._graph = "captured"
    h.set_logit_processors(False)
    assert h._graph is None and h._proc is None and h._feature_key() == (None, False)
    with pytest.raises(ValueError):
        h.set_logprobs(9)


def test_sampler_features_refusal_comes_before_any_buffer(monkeypatch):
    def no_buffers(*a, **k):
        raise AssertionError("a buffer was built before the refusal")

    monkeypatch.setattr(EF.LP, "LogprobBuffers", no_buffers)
    monkeypatch.setattr(EF.PR, "LogitProcessors", no_buffers)
    h = _Refusing()
    with pytest.raises(NotImplementedError, match="no logprobs here"):
        h.set_logprobs(0)
    with pytest.raises(NotImplementedError, match="no logit processors here"):
        h.set_logit_processors(True)
    assert h._lp is None and h._proc is None and h._graph == "captured"
    h.set_logprobs(None)  # switching off is never refused
    h.set_logit_processors(False)
    assert h._graph is None


def _int8(m):
    """every linear an int8 weight-only one, as far as `supports` looks: int8 weight, 16-bit per-column scales"""
    for lin in EF.model_linears(m):
        lin.weight = torch.nn.Parameter(torch.zeros(lin.weight.shape, dtype=torch.int8), requires_grad=False)
        lin.scales = torch.ones(lin.weight.shape[0], dtype=torch.float16)
    return m


def test_weight_refusals_keep_their_texts():
    def batched_q(lin):
        return hasattr(lin, "scales_and_zeros") or hasattr(lin, "scales") or lin.weight.dtype == torch.int8

    def prefill_q(lin):
        return hasattr(lin, "scales_and_zeros") or hasattr(lin, "scales")

    i8 = _int8(_model(caches=False))
    assert EF.dense_16bit_refusal(i8, batched_q, "quantised (int8 / int4) weights are not batched") == \
        BatchedDecodeEngine.supports(i8) == "quantised (int8 / int4) weights are not batched"
    assert EF.dense_16bit_refusal(i8, prefill_q, "quantised weights prefill through the module path") == \
        PrefillEngine.supports(i8) == "quantised weights prefill through the module path"

    mixed = _model(caches=False)
    mixed.layers[1].feed_forward.w2.to(torch.float32)
    assert EF.dense_16bit_refusal(mixed, batched_q, "-") == BatchedDecodeEngine.supports(mixed) == PrefillEngine.supports(mixed) == \
        "weights are not uniformly fp16 / bf16: torch.float16"
    f32 = _model(dtype=torch.float32, caches=False)
    assert EF.dense_16bit_refusal(f32, prefill_q, "-") == BatchedDecodeEngine.supports(f32) == PrefillEngine.supports(f32) == \
        "weights are not uniformly fp16 / bf16: torch.float32"

    cpu = _model(caches=False)
    assert EF.dense_16bit_refusal(cpu, batched_q, "-") == BatchedDecodeEngine.supports(cpu) == PrefillEngine.supports(cpu) == \
        "model is not on a HIP device"
