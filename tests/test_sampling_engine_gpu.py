"""GPU: per-request sampling through the engines (SlotDecodeEngine, DecodeEngine, BatchedDecodeEngine, ContinuousBatcher, generate.py)
on `tiny-test` and a 2-layer model of Llama-2-7B's width.  The truth is the host model (tests/sampling_rule.py) on the logits each
step left.

  1. SlotDecodeEngine stepped without a graph, B = 3 with three different settings: every kept count is one the model allows and
     every token is the model's draw from that kept set (its runner-up where the race is open: at most 2 % of the draws); the
     captured run gives the same tokens;
  2. with every row kept, a request's tokens are those it draws alone on the engine, whatever its slot and its neighbours' settings;
  3. the feature on with every request at the batcher's defaults: the tokens of the feature-off run, bit for bit;
  4. a top_k = 1 request and a top_p = 1e-6 request both reproduce the argmax of each step's logits;
  5. next to logit processors the draw is taken from the adjusted row, and logprobs stay the raw row's;
  6. DecodeEngine and BatchedDecodeEngine on a short run;
  7. generate.py --requests end to end on a file mixing the four fields and "seed";
  8. with the feature off a step launches what it launched before.
"""
import numpy as np
import pytest
import torch

import logprob_rule as LR
import sampler_rule as SR
import sampling_rule as R
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_PRODUCED, BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.continuous import ContinuousBatcher, Request
from teal_amd.gpt_fast.engine import DecodeEngine
from test_logit_engine_gpu import _bits, _calls_of, _main, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_SEQ, STEPS = 64, 20
KW = dict(temperature=0.8, top_k=50)  # what run_steps is given: with the feature on it must not matter

# slot: (prompt, budget, seed, (temperature, top_k, top_p, min_p)); one budget ends mid-run
REQS3 = {
    0: ([5, 9, 300, 9, 17], STEPS + 1, 21, (0.8, 40, 0.9, 0.0)),
    1: ([44], 9, 22, (1.2, 0, 0.7, 0.02)),
    2: ([7, 7, 7, 450, 2, 2, 81, 6, 13, 250, 11], STEPS + 1, 23, (0.6, 0, 1.0, 0.1)),
}


def _skw(s):
    return dict(temperature=s[0], top_k=s[1], top_p=s[2], min_p=s[3])


def _clip(reqs, V):
    return {s: ([t % V for t in p], b, seed, st) for s, (p, b, seed, st) in reqs.items()}


class _Tally:
    def __init__(self):
        self.bad, self.draws, self.open, self.filtered = [], 0, 0, 0

    def check(self, where, row_bits, setting, seed, ctr, got_tok, got_kept):
        T, k, p, m = setting
        _, count, is_open, counts = R.kept(row_bits, False, T, k, p, m)
        if got_kept not in counts:
            self.bad.append((where, "kept", got_kept, counts))
            return
        tok, ru, op = R.draws_from(row_bits, False, got_kept, T, seed, ctr, 1)
        self.draws += 1
        self.open += int(op[0])
        self.filtered += int(got_kept < row_bits.size)
        if not (got_tok == tok[0] or (op[0] and got_tok == ru[0])):
            self.bad.append((where, "token", got_tok, int(tok[0]), int(ru[0]), bool(op[0])))

    def clean(self):
        assert not self.bad, self.bad[:5]
        assert self.open <= 0.02 * self.draws, (self.open, self.draws)


def _admit_all(eng, reqs):
    for s, (prompt, budget, seed, st) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **_skw(st))


def _stepped(eng, reqs, steps, tally):
    ctr = {}
    for s, (prompt, budget, seed, st) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **_skw(st))
        torch.cuda.synchronize()
        tally.check(("admit", s), _bits(eng.admit_logits.view(-1)), st, seed, 0, int(eng.history[s, 0]), int(eng.sampling_kept[s]))
        ctr[s] = 1
    for i in range(steps):
        active = eng.read_state()[SLOT_ACTIVE]
        eng._self_step(**KW)
        torch.cuda.synchronize()
        raw, kept = _bits(eng.logits), eng.sampling_kept.tolist()
        for s, (prompt, budget, seed, st) in reqs.items():
            if (active >> s) & 1:
                tally.check(("step", i, s), raw[s], st, seed, ctr[s], int(eng.tok_buf[s]), kept[s])
                ctr[s] += 1
    state = eng.read_state()
    assert state[SLOT_ACTIVE] == 0
    return {s: eng.read_history(s, state[SLOT_PRODUCED + s]) for s in reqs}


def _run_graph(eng, reqs, steps=STEPS):
    _admit_all(eng, reqs)
    eng.run_steps(steps, use_graph=True, **KW)
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0
    return {s: eng.read_history(s, st[SLOT_PRODUCED + s]) for s in reqs}


@pytest.mark.parametrize("name,n_layer", [("tiny-test", None), ("7B", 2)])
def test_slot_engine_stepped_against_the_model_and_captured(name, n_layer):
    m, ths = _model(name, n_layer, 3)
    reqs = _clip(REQS3, m.config.vocab_size)
    eng = SlotDecodeEngine(m, ths, 3)
    eng.set_sampling_params(True)
    tally = _Tally()
    stepped = _stepped(eng, reqs, STEPS, tally)
    tally.clean()
    assert tally.draws == sum(min(b, STEPS + 1) for _, b, _, _ in reqs.values()) and tally.filtered > 0.9 * tally.draws
    assert _run_graph(eng, reqs) == stepped
    # one graph serves any mix: other settings in the same slots, the same captured step
    g = eng._graph
    other = {s: (p, b, seed, REQS3[(s + 1) % 3][3]) for s, (p, b, seed, _) in reqs.items()}
    again = _run_graph(eng, other)
    assert eng._graph is g and again != stepped
    eng.run_steps(1, temperature=1.7, top_k=3, use_graph=True)  # the scalars a step is given do not re-capture it either
    assert eng._graph is g


def _dense_engine():
    # every row kept: a step's sums do not depend on what the neighbours draw (tests/test_logit_engine_gpu.py says why)
    m, ths = _model("tiny-test", None, 3, sparsity=0.0)
    return SlotDecodeEngine(m, ths, 3)


def test_a_requests_tokens_do_not_depend_on_its_slot_or_its_neighbours():
    eng = _dense_engine()
    eng.set_sampling_params(True)
    V = eng.cfg.vocab_size
    reqs = _clip(REQS3, V)
    together = _run_graph(eng, reqs)
    for s, q in reqs.items():
        alone = _run_graph(eng, {(s + 1) % 3: q})
        assert alone[(s + 1) % 3] == together[s], s
    moved = {0: reqs[2], 1: reqs[0], 2: (reqs[1][0], reqs[1][1], reqs[1][2], (0.3, 5, 0.5, 0.0))}  # and a neighbour with other settings
    got = _run_graph(eng, moved)
    assert got[0] == together[2] and got[1] == together[0] and got[2] != together[1]
    for bad, msg in [(dict(top_p=0.0), "top_p"), (dict(min_p=1.0), "min_p"), (dict(temperature=-1.0), "temperature"), (dict(top_k=-2), "top_k")]:
        with pytest.raises(ValueError, match=msg):
            eng.admit(0, [1, 2], 3, None, 1, **{**KW, **bad})
    assert eng.read_state()[SLOT_ACTIVE] == 0  # refused before anything moved


def test_the_feature_on_at_the_defaults_gives_the_feature_off_runs_tokens():
    eng = _dense_engine()
    eng.set_sampling_params(False)
    plain = {s: (p, b, seed) for s, (p, b, seed, _) in _clip(REQS3, eng.cfg.vocab_size).items()}

    def run():
        for s, (p, b, seed) in plain.items():
            eng.admit(s, p, b, None, seed, **KW)
        eng.run_steps(STEPS, use_graph=True, **KW)
        st = eng.read_state()
        return {s: eng.read_history(s, st[SLOT_PRODUCED + s]) for s in plain}

    off = run()
    with pytest.raises(RuntimeError, match="off"):
        eng.admit(0, [1, 2], 3, None, 1, **KW, top_p=0.9)
    with pytest.raises(RuntimeError, match="off"):
        eng.set_slot_sampling(0, 0.8, 50)
    eng.admit(0, [1, 2], 1, None, 1, **KW, top_p=1.0, min_p=0.0)  # spelled-out "off" needs nothing
    eng.set_sampling_params(True)
    assert run() == off
    assert eng.sampling_params.shape == (3, 4) and eng.sampling_kept.dtype == torch.int32
    # ... and through the batcher: defaults only -> the feature stays off; one request with top_p -> on, the others' tokens stay
    rs = [Request(p, b, seed=seed) for p, b, seed in plain.values()]
    eng.set_sampling_params(False)
    res = ContinuousBatcher(eng, sync_every=4, **KW).run(rs)
    assert res["tokens"] == [off[s] for s in plain] and eng.sampling_params is None
    rs[1] = Request(rs[1].tokens, rs[1].max_new_tokens, seed=rs[1].seed, top_p=0.5)
    res = ContinuousBatcher(eng, sync_every=4, **KW).run(rs)
    assert eng.sampling_params is not None
    assert res["tokens"][0] == off[0] and res["tokens"][2] == off[2] and res["tokens"][1] != off[1]


def test_top_k_1_and_a_tiny_nucleus_both_give_the_argmax():
    m, ths = _model("tiny-test", None, 2)
    eng = SlotDecodeEngine(m, ths, 2)
    eng.set_sampling_params(True)
    eng.admit(0, [5, 9, 300], STEPS + 1, None, 31, temperature=0.8, top_k=1)
    first0 = (eng.admit_logits.float().max().item(), eng.admit_logits[int(eng.history[0, 0])].float().item())
    eng.admit(1, [44, 45], STEPS + 1, None, 32, temperature=1.5, top_k=0, top_p=1e-6)
    first1 = (eng.admit_logits.float().max().item(), eng.admit_logits[int(eng.history[1, 0])].float().item())
    assert first0[0] == first0[1] and first1[0] == first1[1]
    for i in range(STEPS):
        eng._self_step(**KW)
        lg, tok = eng.logits.float(), eng.tok_buf[:2].long()
        assert torch.equal(lg.gather(1, tok.view(2, 1)).view(-1), lg.max(dim=1).values), i
        assert eng.sampling_kept.tolist() == (lg == lg.max(dim=1, keepdim=True).values).sum(1).tolist()  # the maxima, ties whole


def test_next_to_logit_processors_the_draw_is_from_the_adjusted_row():
    m, ths = _model("tiny-test", None, 2)
    eng = SlotDecodeEngine(m, ths, 2)
    eng.set_sampling_params(True)
    eng.set_logit_processors(True)
    eng.set_logprobs(0)
    st = (0.9, 0, 0.8, 0.01)
    eng.admit(0, [5, 9, 300, 9], 12, None, 41, **_skw(st), logit_bias={"77": 200.0})  # far above every logit: that token, kept = 1
    eng.admit(1, [8, 3], 12, None, 42, **_skw(st), frequency_penalty=0.7)
    tally = _Tally()
    torch.cuda.synchronize()
    tally.check("admit", _bits(eng.adj_logits[1]), st, 42, 0, int(eng.history[1, 0]), int(eng.sampling_kept[1]))
    for i in range(11):
        eng._self_step(**KW)
        torch.cuda.synchronize()
        tally.check(i, _bits(eng.adj_logits[1]), st, 42, i + 1, int(eng.tok_buf[1]), int(eng.sampling_kept[1]))
        assert int(eng.tok_buf[0]) == 77 and int(eng.sampling_kept[0]) == 1
        lp = eng._lp.read(0, i + 1, 1)[0]
        truth = LR.logprobs64(SR.decode(_bits(eng.logits[0]), False).astype(np.float64))
        assert LR.close(lp.cpu().numpy()[0], truth[77]) and truth[77] < -1.0  # the MODEL's logprob of the forced token: unlikely
    tally.clean()
    assert eng.read_state()[SLOT_ACTIVE] == 0


def test_decode_engine_and_batched_engine_draw_by_the_model():
    n = 8
    m, ths = _model("tiny-test", None, 1)
    prompt = torch.tensor([5, 9, 300, 9, 17, 44], device=DEV, dtype=torch.int)
    st = (0.9, 30, 0.8, 0.01)
    with torch.no_grad():
        row = m(prompt.view(1, -1), torch.arange(6, device=DEV))[0, -1].clone()
        eng = DecodeEngine(m, ths)
        eng.manual_seed(5)
        first = eng.sample_first(row, **KW).clone()
        off = [int(first)] + eng.decode_n(first, 6, n, drawn=1, **KW).tolist()
        eng.set_sampling_params(True)
        eng.set_slot_sampling(0, KW["temperature"], KW["top_k"])
        eng.manual_seed(5)
        first = eng.sample_first(row, **KW).clone()
        assert [int(first)] + eng.decode_n(first, 6, n, drawn=1, **KW).tolist() == off  # top_p = 1, min_p = 0: the top-k sampler's tokens
        eng.set_slot_sampling(0, *st)
        eng.manual_seed(5)
        first = eng.sample_first(row, temperature=3.0, top_k=1).clone()  # (the scalars do not matter any more)
        torch.cuda.synchronize()
        seed, tally = int(eng.rng_state[0]), _Tally()
        tally.check("first", _bits(row), st, seed, 0, int(first), int(eng.sampling_kept[0]))
        eng.tok_buf.copy_(first.view(1, 1))
        eng.pos_buf.fill_(6)
        toks = [int(first)]
        for i in range(n):
            eng._self_step(**KW)
            torch.cuda.synchronize()
            toks.append(int(eng.tok_buf))
            tally.check(i, _bits(eng.logits.view(-1)), st, seed, i + 1, toks[-1], int(eng.sampling_kept[0]))
        tally.clean()
        eng.manual_seed(5)
        first2 = eng.sample_first(row, **KW).clone()
        assert [int(first2)] + eng.decode_n(first2, 6, n, drawn=1, temperature=2.0, top_k=7).tolist() == toks  # the captured step
    eng.speculating = True  # what SpeculativeDecoder leaves on its draft engine
    with pytest.raises(NotImplementedError, match="speculative"):
        eng.set_sampling_params(True)
    eng.speculating = False
    eng.reduce = lambda t: t  # what tp.apply_tp leaves on a sharded model's engine
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        eng.set_sampling_params(True)
    # the batched engine: three rows, three settings
    B = 3
    mb, thb = _model("tiny-test", None, B)
    engb = BatchedDecodeEngine(mb, thb, B)
    firsts = torch.tensor([5, 9, 300], device=DEV, dtype=torch.int32)
    sts = [(0.9, 30, 0.8, 0.0), (1.0, 0, 1.0, 0.05), (0.7, 10, 0.6, 0.0)]
    engb.set_sampling_params(True)
    for b in range(B):
        engb.set_slot_sampling(b, *sts[b])
    engb.tok_buf[:B].copy_(firsts)
    engb.pos_buf[:B].fill_(0)
    engb.rng_state.copy_(torch.tensor([[3 + b, 0] for b in range(B)], dtype=torch.int64))
    tally = _Tally()
    for i in range(n):
        engb._self_step(**KW)
        torch.cuda.synchronize()
        raw = _bits(engb.logits)
        for b in range(B):
            tally.check((i, b), raw[b], sts[b], 3 + b, i, int(engb.tok_buf[b]), int(engb.sampling_kept[b]))
    tally.clean()
    eager = engb.history[:, :n].clone()
    engb.manual_seed(3)
    assert torch.equal(engb.decode_n(firsts, 0, n, **KW), eager)


def test_with_the_feature_off_a_step_launches_what_it_launched_before():
    B = 3
    m, ths = _model("tiny-test", None, B)
    eng = SlotDecodeEngine(m, ths, B)
    for s, (p, b, seed, _) in _clip(REQS3, m.config.vocab_size).items():
        eng.admit(s, p, b, None, seed, **KW)

    def calls_of(step):
        if eng._samp is not None:
            keep = eng._samp.L
            calls = []
            from test_logit_engine_gpu import _Count
            eng._samp.L = _Count(keep, calls)
            try:
                return _calls_of(eng, step) + calls
            finally:
                eng._samp.L = keep
        return _calls_of(eng, step)

    step = lambda: eng._self_step(**KW)  # noqa: E731
    fresh = calls_of(step)
    n_layers = len(m.layers)
    # embedding rows; per layer qkv, attention, wo, resid, gate|up, down, resid; lm_head and its rounding; B samplers; retire
    assert len(fresh) == 1 + 7 * n_layers + 2 + B + 1 and fresh.count("teal_sample_topk_slot") == B and "teal_sample_rows" not in fresh
    admit = lambda: eng.admit(0, [1, 2, 3], 2, None, 5, **KW)  # noqa: E731
    eng.run_steps(STEPS, use_graph=False, **KW)
    admit_fresh = calls_of(admit)
    assert admit_fresh.count("teal_sample_topk_slot") == 1 and "teal_sample_rows" not in admit_fresh
    eng.run_steps(2, use_graph=False, **KW)
    eng.set_sampling_params(True)
    on = calls_of(step)
    assert len(on) == len(fresh) - B + 1 and on.count("teal_sample_rows") == 1 and "teal_sample_topk_slot" not in on
    admit_on = calls_of(admit)
    assert len(admit_on) == len(admit_fresh) and admit_on.count("teal_sample_rows") == 1 and "teal_sample_topk_slot" not in admit_on
    eng.run_steps(2, use_graph=False, **KW)
    eng.set_sampling_params(False)
    assert calls_of(step) == fresh and calls_of(admit) == admit_fresh and eng.sampling_params is None and eng.sampling_kept is None


def test_generate_requests_end_to_end_with_mixed_sampling(tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text('{"tokens": [1, 2, 3]}\n'
                 '{"tokens": [4], "max_new_tokens": 30, "top_k": 1, "seed": 5}\n'
                 '{"tokens": [4], "max_new_tokens": 30, "top_p": 0.000001, "temperature": 2.0, "seed": 6}\n'
                 '{"tokens": [5, 6, 7, 8, 9], "max_new_tokens": 9, "temperature": 0, "seed": 7}\n'
                 '{"tokens": [10, 11], "max_new_tokens": 20, "min_p": 0.2, "top_p": 0.9, "seed": 8}\n'
                 '{"tokens": [10, 11], "max_new_tokens": 20, "min_p": 0.2, "top_p": 0.9, "seed": 8}\n'
                 '{"tokens": [10, 11], "max_new_tokens": 20, "seed": 8}\n')
    res = _main("--compile", "--requests", str(f), "--batch_size", "2", "--sparsity", "0.0")
    seqs = res["sequences"]
    assert [len(s) for s in seqs] == [12, 30, 30, 9, 20, 20, 20]
    assert seqs[1] == seqs[2]                       # greedy either way: the seeds and temperatures do not matter
    assert seqs[4] == seqs[5] and seqs[4] != seqs[6]  # the same seed and settings: the same tokens, in whatever slot; other settings: others
    plain = _main("--compile", "--requests", str(f), "--batch_size", "2", "--sparsity", "0.0", "--top_p", "0.9", "--min_p", "0.2")
    assert plain["sequences"][6] == seqs[4] and plain["sequences"][1] == seqs[1]  # the flags are the defaults of requests that set none
    # the single-sequence and the --batch_size engine paths take the flags too: a tiny nucleus is greedy, whatever the temperature
    a, b = _main("--compile", "--top_p", "0.000001", new=20), _main("--compile", "--top_p", "0.000001", "--temperature", "1.9", new=20)
    assert a["sequences"][0] == b["sequences"][0]
    a = _main("--compile", "--batch_size", "3", "--top_p", "0.000001", new=20)
    b = _main("--compile", "--batch_size", "3", "--top_p", "0.000001", "--top_k", "7", "--temperature", "1.9", new=20)
    assert a["sequences"][0] == b["sequences"][0]  # (the first new token comes from the sampling launch too)
