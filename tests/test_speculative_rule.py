"""CPU: the accept rule of teal_spec_accept (numpy restatement) against the reference's (torch), and the speculative-decoding
argument checks of generate.main, which refuse before anything is loaded."""
import os

import numpy as np
import pytest
import torch

from spec_rule import accept_numpy, accept_reference_torch, hash3, row_probs, uniform
from teal_amd.gpt_fast import generate as G


@pytest.mark.parametrize("k,V,top_k", [(1, 64, 0), (4, 512, 0), (4, 512, 20), (15, 256, 5)])
def test_numpy_accept_rule_matches_the_reference(k, V, top_k):
    rng = np.random.default_rng(k * 1000 + V + top_k)
    agree = 0
    for r in range(200):
        tq = (rng.standard_normal((k + 1, V)) * 2).astype(np.float16)
        tp = (tq[:k].astype(np.float32) + rng.standard_normal((k, V)).astype(np.float32) * 0.5).astype(np.float16)
        q = np.stack([row_probs(row.view(np.uint16), False, top_k, 0.8) for row in tq])
        p = np.stack([row_probs(row.view(np.uint16), False, top_k, 0.8) for row in tp])
        drafts = np.array([rng.choice(V, p=p[i].astype(np.float64) / p[i].astype(np.float64).sum()) for i in range(k)])
        seed, ctr = 77 + r, 2 * r
        n, tok, near = accept_numpy(q, p, drafts, seed, ctr)
        u = torch.from_numpy(uniform(hash3(seed, ctr, np.arange(k))))
        e = torch.from_numpy((-np.log(uniform(hash3(seed, ctr + 1, np.arange(V))))).astype(np.float32))
        n_ref, tok_ref = accept_reference_torch(torch.from_numpy(q), torch.from_numpy(p), torch.from_numpy(drafts), u, e)
        if near:
            continue
        assert (n, tok) == (n_ref, tok_ref), (r, n, tok, n_ref, tok_ref)
        agree += 1
    assert agree >= 190


def test_zero_draft_probability_is_a_rejection():
    q = np.full((2, 8), 1 / 8, dtype=np.float32)
    p = np.zeros((1, 8), dtype=np.float32)
    p[0, 1] = 1.0
    n, _, _ = accept_numpy(q, p, [3], 1, 0)  # d = 3 has p = 0 under the draft: rejected, whatever u is
    assert n == 0


def _args(*extra):
    return G.build_parser().parse_args(["--device", "cuda", *extra])


@pytest.mark.parametrize("argv,match", [
    (["--checkpoint_path", "a/model.pth", "--draft_checkpoint_path", "nowhere/model.pth"], "not found"),
    (["--synthetic", "tiny-test", "--self_speculate", "--speculate_k", "0"], "1..15"),
    (["--synthetic", "tiny-test", "--self_speculate", "--speculate_k", "16"], "1..15"),
    (["--checkpoint_path", "a/model_int8.pth", "--draft_checkpoint_path", "d/model.pth"], "quantised"),
    (["--checkpoint_path", "a/model.pth", "--self_speculate"], "synthetic"),
])
def test_speculative_arguments_refused_before_loading(argv, match, monkeypatch):
    monkeypatch.setattr(G, "build_synthetic_model", lambda *a, **k: pytest.fail("loaded a model before refusing"))
    monkeypatch.setattr(G, "load_checkpoint_model", lambda *a, **k: pytest.fail("loaded a model before refusing"))
    with pytest.raises(SystemExit, match="speculative decoding") as ei:
        G.main(_args(*argv))
    assert match in str(ei.value)


def test_speculative_refused_under_tensor_parallelism(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="speculative decoding does not run under tensor parallelism"):
        G.main(_args("--synthetic", "tiny-test", "--self_speculate"))


def test_speculative_vocabulary_mismatch_refused(tmp_path):
    t = tmp_path / "Llama-2-7b-chat-hf"
    d = tmp_path / "Meta-Llama-3-8B"
    t.mkdir()
    d.mkdir()
    (t / "model.pth").write_bytes(b"")
    (d / "model.pth").write_bytes(b"")
    with pytest.raises(SystemExit, match="speculative decoding: the draft's vocabulary"):
        G.main(_args("--checkpoint_path", str(t / "model.pth"), "--draft_checkpoint_path", str(d / "model.pth")))


def test_draft_path_equal_to_target_selects_self_speculation(tmp_path):
    t = tmp_path / "Llama-2-7b-chat-hf"
    t.mkdir()
    (t / "model.pth").write_bytes(b"")
    a = _args("--checkpoint_path", str(t / "model.pth"), "--draft_checkpoint_path", str(t / "model.pth"))
    assert G.check_speculative_args(a) == "self"
    assert G.check_speculative_args(_args("--synthetic", "tiny-test")) is None


def test_quantised_target_refused_by_its_directory_name_too(tmp_path):
    """the loader decides int8 / int4 on the whole path (load_checkpoint_model): so does the pre-load check"""
    t = tmp_path / "Llama-2-7b-int8" / "model.pth"
    with pytest.raises(SystemExit, match="speculative decoding verifies with a dense 16-bit target"):
        G.main(_args("--checkpoint_path", str(t), "--draft_checkpoint_path", str(tmp_path / "d" / "model.pth")))


def test_speculative_kernels_do_not_spill_to_scratch(tmp_path):
    """every kernel of teal_speculative.hip compiles for gfx950 with the library's flags and no scratch (private) memory"""
    import re
    import subprocess
    from teal_amd import _lib
    src = os.path.join(_lib.CSRC, "teal_speculative.hip")
    cmd = [_lib._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", f"-I{_lib.INCLUDE}", f"-I{_lib.CSRC}",
           *_lib.NO_PACKED_FP32, _lib.FP_CONTRACT, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "spec.o")]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) >= 8 and len(scratch) == len(names), (len(names), len(scratch))
    assert all(s == 0 for s in scratch), [(n, s) for n, s in zip(names, scratch) if s]
    assert not re.findall(r"VGPRs Spill: [1-9]", r.stderr)
