"""GPU: token log-probabilities through the engines (DecodeEngine, SlotDecodeEngine, ContinuousBatcher) and DecodeEngine.score, on
`tiny-test` and a 2-layer model of Llama-2-7B's width; the truth is the fp64 rule (tests/logprob_rule.py) on the logits each
step left, cloned during an eager run.

  1. DecodeEngine: switching logprobs on changes no token; eager lp / top-5 match the truth step by step; the graph run's bits
     are the eager run's;
  2. SlotDecodeEngine, B = 4: every produced token — the first, from admission, and each request's last included — has the logprob
     of the row that drew it; an empty slot's and a retired slot's tail keep their fill pattern; graph = eager bit for bit;
  3. ContinuousBatcher on the real engine: logprobs=0 changes no token and aligns with "tokens";
  4. score: graph = eager bit for bit, both match the truth of an eager teacher-forced walk, and at thresholds -1 the module
     path's log-softmax within twice the engine-vs-module logit bound.
"""
import numpy as np
import pytest
import torch

import logprob_rule as R
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_PRODUCED, SlotDecodeEngine
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from teal_amd.gpt_fast.engine import DecodeEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODELS = [("tiny-test", None), ("7B", 2)]
KW = dict(temperature=0.8, top_k=50)


def _model(name, n_layer, B, max_seq, sparsity=0.5, seed=3):
    m = G.build_synthetic_model(name, DEV, torch.float16, seed=seed, std=0.05 if name == "tiny-test" else 0.02, n_layer=n_layer)
    ths = G.apply_sparsity(m, sparsity=sparsity, hist_path=None, greedy_lookup=None, synthetic=True, decode_calibration=False)
    m.max_seq_length = -1
    m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
    return m, ths


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _rows64(t):
    return t.view(-1, t.shape[-1]).double().cpu().numpy()


def _fill(eng):
    for t in eng._lp.tensors():
        t.view(torch.int32).fill_(R.NAN_BITS)


@pytest.mark.parametrize("name,n_layer", MODELS)
def test_decode_engine_logprobs(name, n_layer):
    n, top = 12, 5
    m, ths = _model(name, n_layer, 1, 64)
    V = m.config.vocab_size
    prompt = torch.randint(0, V, (6,), device=DEV, dtype=torch.int)
    with torch.no_grad():
        m(prompt.view(1, -1), torch.arange(6, device=DEV))
        eng = DecodeEngine(m, ths)
        first = torch.tensor([[11]], device=DEV, dtype=torch.int)
        eng.manual_seed(5)
        off = eng.decode_n(first, 6, n, **KW)
        eng.set_logprobs(top)
        eng.manual_seed(5)
        on = eng.decode_n(first, 6, n, **KW)
        assert torch.equal(off, on), "switching logprobs on changed the tokens"
        graph = eng.read_logprobs(0, n)
        # the same run eagerly, keeping every step's logits
        _fill(eng)
        eng.manual_seed(5)
        eng.tok_buf.copy_(first)
        eng.pos_buf.fill_(6)
        eng.begin_sequence()
        rows = []
        for _ in range(n):
            eng._self_step(**KW)
            rows.append(eng.logits.view(-1).clone())
        toks = eng.history[:n].tolist()
        eager = eng.read_logprobs(0, n)
    assert toks == on.tolist()
    lp, ids, tlp = (t.cpu().numpy() for t in eager)
    for i in range(n):
        r64 = _rows64(rows[i])[0]
        truth = R.logprobs64(r64)
        assert R.close(lp[i], truth[toks[i]]), (i, lp[i], truth[toks[i]])
        want = R.top_n(r64, top)
        assert ids[i].tolist() == want.tolist() and R.close(tlp[i], truth[want]), (i, R.worst(tlp[i], truth[want]))
    for a, b in zip(graph, eager):
        assert np.array_equal(_bits(a), _bits(b))
    assert (_bits(eng._lp.lp)[0, n:] == R.NAN_BITS).all()  # nothing past the n draws
    with pytest.raises(ValueError, match="0..8"):
        eng.set_logprobs(9)
    eng.set_logprobs(None)
    with pytest.raises(RuntimeError, match="off"):
        eng.read_logprobs(0, 1)


def test_set_logprobs_refuses_tensor_parallel_engines():
    m, ths = _model("tiny-test", None, 1, 64)
    eng = DecodeEngine(m, ths)
    eng.reduce = lambda t: t  # what tp.apply_tp leaves on a sharded model's engine
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        eng.set_logprobs(0)


def _slot_run(eng, reqs, steps, use_graph):
    """admit reqs {slot: (prompt, budget, seed)} and run `steps` steps; eager: one step at a time, returning what each left"""
    _fill(eng)
    admitted, stepped = {}, []
    for s, (prompt, budget, seed) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **KW)
        admitted[s] = eng.admit_logits.view(-1).clone()
    if use_graph:
        eng.run_steps(steps, use_graph=True, **KW)
    else:
        for _ in range(steps):
            active = eng.read_state()[SLOT_ACTIVE]
            eng._self_step(**KW)
            stepped.append((active, eng.logits.clone(), eng.tok_buf.clone()))
    state = eng.read_state()
    return admitted, stepped, state, [t.clone() for t in eng._lp.tensors()], eng.history.clone()


@pytest.mark.parametrize("name,n_layer", MODELS)
def test_slot_engine_logprobs(name, n_layer):
    B, steps, top = 4, 8, 3
    m, ths = _model(name, n_layer, B, 64)
    V = m.config.vocab_size
    g = torch.Generator().manual_seed(7)
    # budgets 9 (ends with the run's last step), 4 (ends mid-run), 7; slot 2 stays empty
    reqs = {0: (torch.randint(0, V, (5,), generator=g).tolist(), 9, 21), 1: (torch.randint(0, V, (1,), generator=g).tolist(), 4, 22),
            3: (torch.randint(0, V, (11,), generator=g).tolist(), 7, 23)}
    eng = SlotDecodeEngine(m, ths, B)
    eng.set_logprobs(top)
    admitted, stepped, state, bufs, hist = _slot_run(eng, reqs, steps, use_graph=False)
    assert state[SLOT_ACTIVE] & 0b1111 == 0
    lp, ids, tlp = (_bits(t) for t in bufs)
    f32 = lambda a: np.asarray(a, dtype=np.int32).view(np.float32)  # noqa: E731
    for s, (_, budget, _) in reqs.items():
        produced = state[SLOT_PRODUCED + s]
        assert produced == budget
        toks = hist[s, :produced].tolist()
        for i in range(produced):
            if i == 0:
                r64 = _rows64(admitted[s])[0]
            else:
                active, logits, tok_buf = stepped[i - 1]
                assert (active >> s) & 1 and int(tok_buf[s]) == toks[i]
                r64 = _rows64(logits)[s]
            truth = R.logprobs64(r64)
            assert R.close(f32(lp[s, i]), truth[toks[i]]), (s, i, f32(lp[s, i]), truth[toks[i]])
            want = R.top_n(r64, top)
            assert ids[s, i].tolist() == want.tolist() and R.close(f32(tlp[s, i]), truth[want]), (s, i)
        # a retired slot's tail keeps the fill pattern
        assert (lp[s, produced:] == R.NAN_BITS).all() and (ids[s, produced:] == R.NAN_BITS).all() and (tlp[s, produced:] == R.NAN_BITS).all()
    assert (lp[2] == R.NAN_BITS).all() and (ids[2] == R.NAN_BITS).all() and (tlp[2] == R.NAN_BITS).all()  # the empty slot
    # the same run through the captured step
    _, _, state_g, bufs_g, hist_g = _slot_run(eng, reqs, steps, use_graph=True)
    assert state_g[SLOT_PRODUCED:SLOT_PRODUCED + B] == state[SLOT_PRODUCED:SLOT_PRODUCED + B] and torch.equal(hist_g, hist)
    for a, b in zip(bufs_g, bufs):
        assert np.array_equal(_bits(a), _bits(b))
    out = eng.read_logprobs(1, 4)
    assert out[0] == f32(lp[1, :4]).tolist() and out[1] == ids[1, :4].tolist() and len(out[2]) == 4 and len(out[2][0]) == top


def test_batched_engine_logprobs():
    B, n, top = 3, 6, 2
    m, ths = _model("tiny-test", None, B, 64)
    from teal_amd.gpt_fast.batched import BatchedDecodeEngine
    eng = BatchedDecodeEngine(m, ths, B)
    first = torch.tensor([5, 9, 300], device=DEV, dtype=torch.int32)
    eng.manual_seed(3)
    off = eng.decode_n(first, 0, n, **KW)
    eng.set_logprobs(top)
    eng.manual_seed(3)
    on = eng.decode_n(first, 0, n, **KW)
    assert torch.equal(off, on)
    graph = eng.read_logprobs(n)
    eng.manual_seed(3)
    eng.tok_buf[:B].copy_(first)
    eng.pos_buf[:B].fill_(0)
    eng.rng_state.copy_(torch.tensor([[3 + b, 0] for b in range(B)], dtype=torch.int64))
    _fill(eng)
    rows = []
    for _ in range(n):
        eng._self_step(**KW)
        rows.append(eng.logits.clone())
    eager = eng.read_logprobs(n)
    assert torch.equal(eng.history[:, :n], on)
    lp, ids, tlp = (t.cpu().numpy() for t in eager)
    assert lp.shape == (B, n) and ids.shape == (B, n, top)
    for i in range(n):
        for b in range(B):
            r64 = _rows64(rows[i])[b]
            truth = R.logprobs64(r64)
            assert R.close(lp[b, i], truth[int(on[b, i])]) and ids[b, i].tolist() == R.top_n(r64, top).tolist()
            assert R.close(tlp[b, i], truth[ids[b, i]])
    for a, b in zip(graph, eager):
        assert np.array_equal(_bits(a), _bits(b))


def test_continuous_batcher_logprobs_on_the_real_engine():
    B = 4
    g = torch.Generator().manual_seed(11)
    reqs = [Request(torch.randint(0, 512, (int(t),), generator=g).tolist(), int(n))
            for t, n in zip(torch.randint(1, 20, (6,), generator=g), torch.randint(2, 12, (6,), generator=g))]
    max_seq = max(len(r.tokens) + r.max_new_tokens for r in reqs)
    m, ths = _model("tiny-test", None, B, max_seq)
    eng = SlotDecodeEngine(m, ths, B)
    a = ContinuousBatcher(eng, sync_every=3, **KW).run(reqs)
    b = ContinuousBatcher(eng, sync_every=3, logprobs=0, **KW).run(reqs)
    assert "logprobs" not in a and a["tokens"] == b["tokens"] and "top_logprobs" not in b
    assert [len(x) for x in b["logprobs"]] == [len(t) for t in b["tokens"]] == [r.max_new_tokens for r in reqs]
    assert all(isinstance(v, float) and v <= 0.0 for x in b["logprobs"] for v in x)
    c = ContinuousBatcher(eng, sync_every=3, logprobs=2, **KW).run(reqs)
    assert c["tokens"] == a["tokens"] and c["logprobs"] == b["logprobs"]
    for lps, alts in zip(c["logprobs"], c["top_logprobs"]):
        assert len(alts) == len(lps) and all(len(x) == 2 and x[0][1] >= x[1][1] and x[0][1] >= lp for x, lp in zip(alts, lps))


def test_score_graph_eager_truth_and_module_path():
    T = 12
    m, ths = _model("tiny-test", None, 1, 64)
    tokens = torch.randint(0, 512, (T,), dtype=torch.int32)
    with torch.no_grad():
        eng = DecodeEngine(m, ths)
        a = eng.score(tokens, use_graph=True)
        b = eng.score(tokens, use_graph=False)
        assert a.shape == (T - 1,) and a.dtype == torch.float32 and np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(eng.score(tokens)), _bits(a))  # the cached graph, again
        # the truth: an eager teacher-forced walk over the same positions
        dev_toks = tokens.to(DEV)
        truth = []
        for p in range(T - 1):
            logits = eng(dev_toks[p].view(1, 1), torch.tensor([p], device=DEV, dtype=torch.int32))
            truth.append(R.logprobs64(_rows64(logits)[0])[int(tokens[p + 1])])
        assert R.close(a.cpu().numpy(), truth), R.worst(a.cpu().numpy(), truth)
        with pytest.raises(ValueError, match="score"):
            eng.score(tokens[:1])
        with pytest.raises(ValueError, match="score"):
            eng.score(torch.zeros(66, dtype=torch.int32))
        # every row kept: against the module path's fp32 log-softmax, step by step (the op-by-op path on the same weights)
        eng.set_thresholds([{k: -1.0 for k in t} for t in ths])
        dense = eng.score(tokens).cpu().numpy()
        ref, rths = _model("tiny-test", None, 1, 64, sparsity=0.0)
        assert all(v == -1.0 for t in rths for v in t.values())
        ref.fused_decode = False
        for p in range(T - 1):
            lg = ref(dev_toks[p].view(1, 1), torch.tensor([p], device=DEV, dtype=torch.int32)).float().view(-1)
            want = float(torch.log_softmax(lg, dim=-1)[int(tokens[p + 1])])
            # tests/test_engine.py holds the engine's logits to the module path's within 6e-3 (1 + |logit|) in fp16 on this model;
            # log-softmax moves by at most twice the sup-norm change of the logits
            bound = 2 * 6e-3 * (1.0 + float(lg.abs().max()))
            assert abs(float(dense[p]) - want) <= bound, (p, float(dense[p]), want, bound)
        assert not np.array_equal(dense, a.cpu().numpy())  # (the sparse score above really ran sparse)


def _main(*extra):
    return G.main(G.build_parser().parse_args(["--device", "cuda", "--synthetic", "tiny-test", "--sparsity", "0.5", "--num_samples", "1",
                                               "--max_new_tokens", "9", *extra]))


def test_generate_logprobs_on_the_engine_paths(tmp_path):
    plain = _main("--compile")
    one = _main("--compile", "--logprobs", "2")
    assert one["sequences"] == plain["sequences"] and "logprobs" not in plain
    assert one["logprob_offset"] == [6] and len(one["logprobs"][0]) == 9 and all(v <= 0.0 for v in one["logprobs"][0])  # all 9 new tokens
    for tok, lp, alts in zip(one["sequences"][0][6:], one["logprobs"][0], one["top_logprobs"][0]):
        assert len(alts) == 2 and alts[0][1] >= alts[1][1] and alts[0][1] >= lp and (tok != alts[0][0] or lp == alts[0][1])
    assert "top_logprobs" not in _main("--engine", "--logprobs", "0")
    bat = _main("--compile", "--batch_size", "3", "--logprobs", "1")
    assert bat["logprob_offset"] == 7 and [len(x) for x in bat["logprobs"][0]] == [8, 8, 8] and len(bat["top_logprobs"][0][2][7]) == 1
    assert bat["sequences"] == _main("--compile", "--batch_size", "3")["sequences"]
    f = tmp_path / "reqs.jsonl"
    f.write_text('{"tokens": [1, 2, 3]}\n{"tokens": [4], "max_new_tokens": 3}\n{"tokens": [5, 6, 7, 8, 9], "max_new_tokens": 12}\n')
    req = _main("--compile", "--requests", str(f), "--batch_size", "2", "--logprobs", "3")
    assert [len(x) for x in req["logprobs"]] == [len(t) for t in req["sequences"]] == [9, 3, 12]
    assert all(len(alts) == 3 for x in req["top_logprobs"] for alts in x)


def test_score_tool_end_to_end(tmp_path, capsys):
    from teal_amd.gpt_fast import score as S
    f = tmp_path / "toks.jsonl"
    g = torch.Generator().manual_seed(2)
    f.write_text("\n".join('{"tokens": %s}' % torch.randint(0, 512, (n,), generator=g).tolist() for n in (40, 7, 1, 17)) + "\n")
    res = S.main(S.build_parser().parse_args(["--synthetic", "tiny-test", "--sparsity", "0.5", "--tokens", str(f), "--window", "16"]))
    # 40 -> 16 + 16 + 8, 7, (1: nothing), 17 -> 16 + (1: nothing): 5 windows, 15 + 15 + 7 + 6 + 15 scored tokens
    assert res["windows"] == 5 and res["scored_tokens"] == 58 and res["window"] == 16
    # random weights: both near the uniform model's 512, and sparsity moves the number
    assert 100 < res["perplexity_dense"] < 2000 and 100 < res["perplexity"] < 2000 and res["perplexity"] != res["perplexity_dense"]
    out = capsys.readouterr().out
    assert "perplexity at sparsity 0.5" in out and "every row kept" in out
