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


# ---- the draw chain: every launch of a draw, in order, with the arguments the engines used to pass by hand ----------------------
class _Rec:
    """a library handle that logs (entry point, arguments) and reports success"""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return lambda *a: self._log.append((name, a)) or 0


class _DrawHost(_Host):
    """four sequences as the batched engines keep them; the fused top-k sampler hook records its call"""

    def __init__(self, log):
        super().__init__()
        self._feature_rows, self._log = 4, log
        self.code = 1
        self.history = torch.zeros(4, 5, dtype=torch.int32)
        self.logits = torch.zeros(4, 16, dtype=torch.float16)
        self.rng_state = torch.zeros(4, 2, dtype=torch.int64)
        self.tok_buf, self.pos_buf = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)

    def _sample_row(self, row, logits, temperature, top_k, feed, st):
        self._log.append(("hook", (row, logits.data_ptr(), temperature, top_k, feed, st)))


ADDR, ST = 0x7F00DEAD0000, 77
DRAW_SHAPES = {"step": (3, 0, None), "slot step": (3, 0, ADDR), "admission": (1, 2, ADDR)}


@pytest.mark.parametrize("shape", list(DRAW_SHAPES))
@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("processors", [False, True])
@pytest.mark.parametrize("logprobs", [False, True])
def test_draw_chain_issues_the_launches_in_order_with_their_arguments(no_library, logprobs, processors, sampling, shape):
    rows, row0, active = DRAW_SHAPES[shape]
    log = []
    h = _DrawHost(log)
    if active is not None:
        h._active = active
    if logprobs:
        h.set_logprobs(2)
        h._lp.L = _Rec(log)
    if processors:
        h.set_logit_processors(True)
        h._proc.L = _Rec(log)
    if sampling:
        h.set_sampling_params(True)
        h._samp.L = _Rec(log)
    V, step = 16, rows > 1
    if step:  # a step's rows: the engine's buffers, rows V apart, each row's fed token counted
        logits, stride, count = h.logits, V, True
        rng, tok, pos, hist = h.rng_state, h.tok_buf, h.pos_buf, h.history
    else:     # one request's first draw: its logits row as it stands, nothing counted
        logits, stride, count = torch.zeros(V, dtype=torch.float16), 0, False
        rng, tok, pos, hist = h.rng_state[row0], h.tok_buf[row0:], h.pos_buf[row0:], h.history[row0]
    h._draw(logits, stride, rows, 0.7, 40, rng, tok, pos, hist, count, row0=row0, st=ST)

    want = []
    src = logits
    if processors:
        p = h._proc
        want.append(("teal_logit_adjust", (logits.data_ptr(), stride, V, p.code, rows, tok.data_ptr(), int(count), p.state[row0].data_ptr(),
                                           p.params[row0].data_ptr(), p.bias[row0].data_ptr(), p.adj[row0].data_ptr(), V, active, row0, ST)))
        src = p.adj[row0:]
        assert src.data_ptr() != logits.data_ptr()
    if sampling:
        s = h._samp
        want.append(("teal_sample_rows", (src.data_ptr(), stride, V, s.code, rows, s.params[row0].data_ptr(), rng.data_ptr(), tok.data_ptr(),
                                          pos.data_ptr(), hist.data_ptr(), 5, s.kept[row0:].data_ptr(), active, row0, ST)))
    else:
        want += [("hook", (row0 + r, (src[r] if step or processors else src).data_ptr(), 0.7, 40, True, ST)) for r in range(rows)]
    if logprobs:
        b = h._lp
        want.append(("teal_token_logprobs", (logits.data_ptr(), stride, V, h.code, rows, tok.data_ptr(), rng.data_ptr(), b.lp[row0].data_ptr(), 5, 2,
                                             b.top_ids[row0].data_ptr(), b.top_lp[row0].data_ptr(), active, row0, ST)))
    assert log == want
    assert len(log) == int(processors) + (1 if sampling else rows) + int(logprobs)


def test_draw_chain_without_a_loop_state_feed_counts_the_fed_buffer(no_library):
    """DecodeEngine.sample_first's shape: the token goes to a buffer of its own, no position or history moves, and the processors
    are still handed the buffer the step is fed from"""
    log = []
    h = _DrawHost(log)
    for on in (lambda: h.set_logprobs(0), lambda: h.set_logit_processors(True)):
        on()
    h._lp.L, h._proc.L = _Rec(log), _Rec(log)
    row, token = torch.zeros(16, dtype=torch.float16), torch.zeros(1, dtype=torch.int32)
    h._draw(row, 0, 1, 0.8, 200, h.rng_state[0], token, None, None, False, fed=h.tok_buf, st=ST)
    (n0, a0), (n1, a1), (n2, a2) = log
    assert (n0, n1, n2) == ("teal_logit_adjust", "hook", "teal_token_logprobs")
    assert a0[0] == row.data_ptr() and a0[5] == h.tok_buf.data_ptr() and a0[6] == 0 and a0[12:] == (None, 0, ST)
    assert a1 == (0, h._proc.adj[0].data_ptr(), 0.8, 200, False, ST)
    assert a2[0] == row.data_ptr() and a2[5] == token.data_ptr() and a2[9] == 0 and a2[10] is None and a2[11] is None
    h.set_sampling_params(True)
    h._samp.L = _Rec(log)
    del log[:]
    h._draw(row, 0, 1, 0.8, 200, h.rng_state[0], token, None, None, False, fed=h.tok_buf, st=ST)
    assert [n for n, _ in log] == ["teal_logit_adjust", "teal_sample_rows", "teal_token_logprobs"]
    assert log[1][1][7:11] == (token.data_ptr(), None, None, 5)


# ---- generate.py: the refusals the engine-path features share keep their texts ---------------------------------------------------
_FLAGS = {"logprobs": dict(logprobs=2), "processors": dict(repetition_penalty=1.3), "sampling": dict(top_p=0.9)}
_REASONS = {"speculative": dict(self_speculate=True), "tensor parallel": {}, "no thresholds": dict(dense=True), "no engine": dict(compile=False)}
_PEN = "--repetition_penalty / --presence_penalty / --frequency_penalty"
REFUSALS = {
    ("logprobs", "speculative"): "--logprobs does not combine with speculative decoding",
    ("logprobs", "tensor parallel"): "--logprobs does not run under tensor parallelism (a rank's lm_head holds a slice of the vocabulary)",
    ("logprobs", "no thresholds"): "--logprobs needs TEAL thresholds (--hist_path, or --synthetic): the fused engines run patched models only",
    ("logprobs", "no engine"): "--logprobs needs a fused engine (--compile or --engine, without --no_engine, or --requests): the module "
                               "path returns token ids only",
    ("processors", "speculative"): _PEN + " do not combine with speculative decoding (the accept rule compares the models' own distributions)",
    ("processors", "tensor parallel"): _PEN + " do not run under tensor parallelism (a rank's lm_head holds a slice of the vocabulary)",
    ("processors", "no thresholds"): _PEN + " need TEAL thresholds (--hist_path, or --synthetic): the fused engines run patched models only",
    ("processors", "no engine"): _PEN + " need a fused engine (--compile or --engine, without --no_engine, or --requests): the module "
                                        "path samples from the raw logits",
    ("sampling", "speculative"): "--top_p / --min_p do not combine with speculative decoding (the accept rule compares the models' distributions "
                                 "under one temperature and top_k)",
    ("sampling", "tensor parallel"): "--top_p / --min_p do not run under tensor parallelism (a rank's lm_head holds a slice of the vocabulary)",
    ("sampling", "no thresholds"): "--top_p / --min_p need TEAL thresholds (--hist_path, or --synthetic): the fused engines run patched models only",
    ("sampling", "no engine"): "--top_p / --min_p need a fused engine (--compile or --engine, without --no_engine, or --requests): the module "
                               "path's sampler knows temperature and top_k only",
}


@pytest.mark.parametrize("feature,reason", list(REFUSALS))
def test_engine_path_refusals_keep_their_texts(monkeypatch, feature, reason):
    from teal_amd.gpt_fast import generate as G
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "2" if reason == "tensor parallel" else "1")
    base = dict(draft_checkpoint_path=None, self_speculate=False, dense=False, synthetic="tiny-test", hist_path=None, requests=None,
                no_engine=False, compile=True, engine=False)
    args = types.SimpleNamespace(**{**base, **_FLAGS[feature], **_REASONS[reason]})
    check = {"logprobs": G.check_logprobs_args, "processors": G.check_processor_args, "sampling": G.check_sampling_args}[feature]
    with pytest.raises(SystemExit) as e:
        check(args)
    assert str(e.value) == REFUSALS[feature, reason]
    ok = types.SimpleNamespace(**{**base, **_FLAGS[feature]})
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert check(ok) == {"logprobs": 2, "processors": {"repetition_penalty": 1.3}, "sampling": {"top_p": 0.9, "min_p": 0.0}}[feature]


# ---- scripts/: the four feature benches keep their command line -----------------------------------------------------------------
BENCH_OPTIONS = """\
options:
  -h, --help            show this help message and exit
  --synthetic SYNTHETIC
  --precision {fp16,bf16}
  --sparsity SPARSITY
  --n_layer N_LAYER
  --steps STEPS
  --pos POS             position of the first timed step
  --chain CHAIN         leg 3: launches per graph
  --legs LEGS
  --settings SETTINGS
  --note NOTE           a line for the head of the record (e.g. which %s
                        this is)
  --out OUT             also append the record to this file
"""


@pytest.mark.parametrize("script,what", [("logprobs_bench", "tree"), ("logit_processors_bench", "tree"), ("sampling_bench", "tree"),
                                         ("stop_bench", "build")])
def test_feature_benches_answer_help_with_their_options(script, what):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, COLUMNS="80", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device to touch)
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", script + ".py"), "--help"], capture_output=True, text=True, env=env,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    usage, _, options = out.stdout.partition("\noptions:\n")
    assert usage.split() == (f"usage: {script}.py [-h] [--synthetic SYNTHETIC] [--precision {{fp16,bf16}}] [--sparsity SPARSITY] [--n_layer N_LAYER] "
                             "[--steps STEPS] [--pos POS] [--chain CHAIN] [--legs LEGS] [--settings SETTINGS] [--note NOTE] [--out OUT]").split()
    assert "options:\n" + options == BENCH_OPTIONS % what
