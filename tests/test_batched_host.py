"""CPU: batched decode (teal_amd/csrc/teal_batched.hip, teal_amd/gpt_fast/batched.py) — what needs no GPU.

  * every kernel of teal_batched.hip compiles for gfx950 with the library's flags and no scratch memory;
  * the numpy restatement of the rule (tests/batched_rule.py): per-sequence masks, the union, its expected size;
  * BatchedDecodeEngine.supports names the reason for each model it cannot run;
  * generate.py --batch_size refuses the combinations it does not support, before loading anything.
"""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from batched_rule import batched_gemv, keep_masks, union_rows
from teal_amd import _lib
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import BatchedDecodeEngine


def test_batched_kernels_do_not_spill_to_scratch(tmp_path):
    src = os.path.join(_lib.CSRC, "teal_batched.hip")
    cmd = [_lib._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", f"-I{_lib.INCLUDE}", f"-I{_lib.CSRC}",
           *_lib.NO_PACKED_FP32, _lib.FP_CONTRACT, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "b.o")]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) >= 30 and len(scratch) == len(names), (len(names), len(scratch))
    assert all(s == 0 for s in scratch), [(n, s) for n, s in zip(names, scratch) if s]
    assert not re.findall(r"VGPRs Spill: [1-9]", r.stderr)


def test_batched_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(_lib.INCLUDE, "teal_hip.h")).read()
    for name in ("teal_batched_sparse_gemm", "teal_batched_round_rows", "teal_batched_decode_attention_ws_bytes",
                 "teal_batched_decode_attention"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\(", hdr), name
    assert "teal_batched.hip" in _lib.SOURCES


def test_rule_masks_each_sequence_by_its_own_activations():
    rng = np.random.default_rng(0)
    Z, N, B = 64, 16, 3
    x = rng.standard_normal((B, Z)).astype(np.float32)
    W = rng.standard_normal((N, Z))
    tau = 0.7
    y = batched_gemv(W, x, [N], [tau])
    for b in range(B):
        keep = np.abs(x[b]) > tau
        assert np.allclose(y[b], W[:, keep] @ x[b, keep].astype(np.float64))
    u = union_rows(keep_masks(x, tau))
    assert u.sum() == (np.abs(x) > tau).any(0).sum()


def test_union_grows_like_one_minus_half_to_the_b():
    rng = np.random.default_rng(1)
    Z = 200000
    for B in (1, 2, 4, 8):
        x = rng.standard_normal((B, Z)).astype(np.float32)
        tau = float(np.quantile(np.abs(x), 0.5))
        frac = union_rows(keep_masks(x, tau)).mean()
        assert abs(frac - (1 - 0.5 ** B)) < 0.01, (B, frac)


def _Lin(n, z, dt=torch.float16):
    return argparse.Namespace(weight=torch.zeros(n, z, dtype=dt), in_features=z, out_features=n)


def _fake_model(dim=256, n_head=4, n_kv=2, inter=512, vocab=512, B=4, tp=1, int8=False, cuda=False):
    hd = dim // n_head

    class Cfg:
        pass
    cfg = Cfg()
    cfg.dim, cfg.n_head, cfg.n_local_heads, cfg.head_dim, cfg.vocab_size = dim, n_head, n_kv, hd, vocab
    layer = argparse.Namespace()
    layer.attention = argparse.Namespace(wqkv=_Lin(dim + 2 * n_kv * hd, dim), wo=_Lin(dim, dim))
    layer.feed_forward = argparse.Namespace(w1=_Lin(inter, dim), w3=_Lin(inter, dim), w2=_Lin(dim, inter))
    kc = torch.zeros(B, n_kv, 16, hd, dtype=torch.float16)
    layer.attention.kv_cache = argparse.Namespace(k_cache=kc, v_cache=kc.clone())
    m = argparse.Namespace(config=cfg, layers=[layer], output=_Lin(vocab, dim), tp_world=tp, freqs_cis=torch.zeros(16, hd // 2, 2, dtype=torch.float16))
    if int8:
        layer.attention.wo.scales = torch.ones(dim)
    if cuda:  # (the device check comes before the shape checks: a CPU model stops there)
        for lin in (layer.attention.wqkv, layer.attention.wo, layer.feed_forward.w1, layer.feed_forward.w3, layer.feed_forward.w2, m.output):
            lin.weight = argparse.Namespace(dtype=lin.weight.dtype, is_cuda=True, shape=lin.weight.shape)
    return m


def test_supports_names_each_reason():
    assert "tensor-parallel" in BatchedDecodeEngine.supports(_fake_model(tp=2))
    assert "quantised" in BatchedDecodeEngine.supports(_fake_model(int8=True))
    assert "HIP device" in BatchedDecodeEngine.supports(_fake_model())
    assert BatchedDecodeEngine.supports(_fake_model(cuda=True)) is None
    assert "contract" in BatchedDecodeEngine.supports(_fake_model(dim=320, n_head=5, cuda=True))
    assert "contract" in BatchedDecodeEngine.supports(_fake_model(vocab=520, cuda=True))
    assert "batch size 9" in BatchedDecodeEngine.supports(_fake_model(B=9, cuda=True))
    m = _fake_model(cuda=True)
    m.layers[0].attention.kv_cache = None
    assert "KV caches" in BatchedDecodeEngine.supports(m)
    m = _fake_model(cuda=True)
    m.freqs_cis = None
    assert "caches are not set up" in BatchedDecodeEngine.supports(m)


def _args(*extra):
    return G.build_parser().parse_args(["--device", "cuda", *extra])


@pytest.mark.parametrize("extra,msg", [
    (("--synthetic", "tiny-test", "--batch_size", "4", "--self_speculate"), "speculative"),
    (("--synthetic", "tiny-test", "--batch_size", "9"), "1..8"),
    (("--synthetic", "tiny-test", "--batch_size", "2", "--interactive"), "interactive"),
    (("--checkpoint_path", "ck/Llama-2-7b-int8/model.pth", "--batch_size", "2"), "16-bit"),
    (("--checkpoint_path", "ck/Llama-2-7b-int4/model.pth", "--batch_size", "2"), "16-bit"),
])
def test_generate_refuses_incompatible_flags(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        G.main(_args(*extra))


def test_generate_refuses_batched_tensor_parallel(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor parallelism"):
        G.check_batched_args(_args("--synthetic", "tiny-test", "--batch_size", "2"))


def test_batch_size_one_is_the_default():
    assert _args().batch_size == 1 and G.check_batched_args(_args()) == 1
