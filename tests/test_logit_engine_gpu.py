"""GPU: per-request logit processors through the engines (SlotDecodeEngine, DecodeEngine, BatchedDecodeEngine, ContinuousBatcher,
generate.py) on `tiny-test` and a 2-layer model of Llama-2-7B's width.  The truth is the host rule (tests/logit_rule.py) applied
to the logits each step left, and the sampler's host model (tests/sampler_rule.py) on the adjusted bits.

  1. SlotDecodeEngine stepped without a graph, B = 3 with different controls per slot: after every step the state table is the
     prompt bits + the history's counts, adj_logits is the rule on engine.logits bit for bit, and each token is the host model's
     draw from the adjusted bits (its runner-up where the model calls the draw open: at most 2 % of the draws);
  2. the captured run gives the stepped run's tokens, state table and adjusted rows;
  3. a request without controls next to requests with controls gets the tokens it gets with the feature off, in any slot;
  4. a frequency penalty large enough to clamp: no token repeats over the budget, and the same request without it does repeat;
  5. logprobs next to processors are the logprob rule on the RAW logits;
  6. a prefix request's prompt bits cover the prefix;
  7. DecodeEngine and BatchedDecodeEngine: the adjust-and-draw check on a short run, and decode_n's graph gives the same tokens;
  8. generate.py --requests end to end on a file that mixes the controls; with the feature off a step launches what it did.
"""
import functools

import numpy as np
import pytest
import torch

import logit_rule as R
import logprob_rule as LR
import sampler_rule as SR
from teal_amd.gpt_fast import generate as G
from teal_amd.gpt_fast.batched import SLOT_ACTIVE, SLOT_PRODUCED, BatchedDecodeEngine, SlotDecodeEngine
from teal_amd.gpt_fast.engine import DecodeEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(temperature=0.8, top_k=50)
MAX_SEQ, STEPS = 64, 24


def _model(name, n_layer, B, max_seq=MAX_SEQ, sparsity=0.5, seed=3):
    m = G.build_synthetic_model(name, DEV, torch.float16, seed=seed, std=0.05 if name == "tiny-test" else 0.02, n_layer=n_layer)
    ths = G.apply_sparsity(m, sparsity=sparsity, hist_path=None, greedy_lookup=None, synthetic=True, decode_calibration=False)
    m.max_seq_length = -1
    m.setup_caches(max_batch_size=B, max_seq_length=max_seq)
    return m, ths


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bias_bits(V, logit_bias):
    if not logit_bias:
        return np.zeros(V, dtype=np.uint16)
    a = np.zeros(V, dtype=np.float32)
    for k, v in logit_bias.items():
        a[int(k)] = v
    return R.encode(a, False)


def _rule(row_bits, state, c):
    return R.adjust(row_bits, False, state, c.get("repetition_penalty", 1.0), c.get("presence_penalty", 0.0), c.get("frequency_penalty", 0.0),
                    _bias_bits(row_bits.size, c.get("logit_bias")))


class _Tally:
    """what a checked run found: mismatches by kind, and how many draws the sampler's model called open"""

    def __init__(self):
        self.adjust, self.state, self.draw, self.draws, self.open = [], [], [], 0, 0

    def check_draw(self, where, adj_bits, seed, ctr, got):
        tok, ru, is_open = SR.draw(adj_bits, False, KW["top_k"], KW["temperature"], seed, ctr)
        self.draws += 1
        self.open += int(is_open)
        if not (got == tok or (is_open and got == ru)):
            self.draw.append((where, got, tok, ru, is_open))

    def check_rows(self, where, got_adj, want_adj, got_state, want_state):
        if not np.array_equal(got_adj, want_adj):
            self.adjust.append((where, int((got_adj != want_adj).sum())))
        if not np.array_equal(got_state, want_state):
            self.state.append((where, int((got_state != want_state).sum())))

    def clean(self):
        assert not self.adjust, self.adjust[:5]
        assert not self.state, self.state[:5]
        assert not self.draw, self.draw[:5]
        assert self.open <= 0.02 * self.draws, (self.open, self.draws)


REQS3 = {  # slot: (prompt, budget, seed, controls); every budget ends within STEPS steps, one mid-run
    0: ([5, 9, 300, 9, 17], STEPS + 1, 21, dict(repetition_penalty=1.3, frequency_penalty=0.2)),
    1: ([44], 12, 22, dict(presence_penalty=0.5, logit_bias={"3": 4.0, "100": -100.0, "101": -100.0})),
    2: ([7, 7, 7, 450, 2, 2, 81, 6, 13, 250, 11], STEPS + 1, 23, dict()),
}


def _clip(reqs, V):
    return {s: ([t % V for t in p], b, seed, {k: ({str(int(i) % V): v for i, v in c.items()} if k == "logit_bias" else c) for k, c in ctl.items()})
            for s, (p, b, seed, ctl) in reqs.items()}


def _admit_all(eng, reqs):
    for s, (prompt, budget, seed, ctl) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **KW, **ctl)


def _stepped(eng, reqs, steps, tally, lp_top=None):
    """admit `reqs` and run `steps` eager steps, holding every admission and every step to the rules; returns (history, state
    table, adjusted rows) as the run left them"""
    V, B = eng.cfg.vocab_size, eng.B
    state = np.zeros((B, V), dtype=np.int32)
    adj_prev = _bits(eng._proc.adj).copy()
    ctr = {}
    lp_bad = []

    def check_lp(where, s, raw_bits, tok, i):
        if lp_top is None:
            return
        lp, ids, tlp = eng._lp.read(s, i, 1)
        truth = LR.logprobs64(R.decode(raw_bits, False).astype(np.float64))
        want = LR.top_n(R.decode(raw_bits, False).astype(np.float64), lp_top)
        if not (LR.close(lp.cpu().numpy()[0], truth[tok]) and ids[0].tolist() == want.tolist() and LR.close(tlp[0].cpu().numpy(), truth[want])):
            lp_bad.append((where, float(lp[0]), float(truth[tok])))

    for s, (prompt, budget, seed, ctl) in reqs.items():
        eng.admit(s, prompt, budget, None, seed, **KW, **ctl)
        torch.cuda.synchronize()
        state[s] = R.prompt_state(V, prompt)  # the first draw counts nothing
        raw = _bits(eng.admit_logits.view(-1))
        want = _rule(raw, state[s], ctl)
        got_adj, got_state = _bits(eng._proc.adj), eng._proc.state.cpu().numpy()
        adj_prev[s] = want
        tally.check_rows(("admit", s), got_adj, adj_prev, got_state, state)
        tok = int(eng.history[s, 0])
        tally.check_draw(("admit", s), got_adj[s], seed, 0, tok)
        check_lp(("admit", s), s, raw, tok, 0)
        ctr[s] = 1
    for i in range(steps):
        active = eng.read_state()[SLOT_ACTIVE]
        fed = eng.tok_buf.tolist()
        eng._self_step(**KW)
        torch.cuda.synchronize()
        raw = _bits(eng.logits)
        got_adj, got_state = _bits(eng._proc.adj), eng._proc.state.cpu().numpy()
        for s, (prompt, budget, seed, ctl) in reqs.items():
            if (active >> s) & 1:
                state[s] = R.count(state[s], fed[s])
                adj_prev[s] = _rule(raw[s], state[s], ctl)
        tally.check_rows(("step", i), got_adj, adj_prev, got_state, state)  # (inactive and empty slots: nothing moved)
        for s, (prompt, budget, seed, ctl) in reqs.items():
            if (active >> s) & 1:
                tok = int(eng.tok_buf[s])
                tally.check_draw(("step", i, s), got_adj[s], seed, ctr[s], tok)
                check_lp(("step", i, s), s, raw[s], tok, ctr[s])
                ctr[s] += 1
    st = eng.read_state()
    hist = eng.history.cpu().numpy().copy()
    for s, (prompt, budget, seed, ctl) in reqs.items():  # the table from the history alone: every token but the last was fed
        n = st[SLOT_PRODUCED + s]
        assert n == min(budget, steps + 1) == ctr[s]
        want = R.prompt_state(V, prompt)
        for t in hist[s, :n - 1]:
            want = R.count(want, int(t))
        assert np.array_equal(eng._proc.state[s].cpu().numpy(), want), s
    return hist, eng._proc.state.cpu().numpy().copy(), _bits(eng._proc.adj).copy(), lp_bad


@functools.lru_cache(maxsize=None)
def _slot_runs(name, n_layer):
    """the stepped run and the captured run of REQS3 on one engine, each from fresh admissions"""
    m, ths = _model(name, n_layer, 3)
    reqs = _clip(REQS3, m.config.vocab_size)
    eng = SlotDecodeEngine(m, ths, 3)
    eng.set_logit_processors(True)
    eng.set_logprobs(2)
    tally = _Tally()
    stepped = _stepped(eng, reqs, STEPS, tally, lp_top=2)
    lp_stepped = [t.clone() for t in eng._lp.tensors()]
    assert eng.read_state()[SLOT_ACTIVE] == 0
    _admit_all(eng, reqs)
    eng.run_steps(STEPS, use_graph=True, **KW)
    torch.cuda.synchronize()
    graph = (eng.history.cpu().numpy().copy(), eng._proc.state.cpu().numpy().copy(), _bits(eng._proc.adj).copy())
    return dict(tally=tally, stepped=stepped, graph=graph, reqs=reqs, lp_stepped=lp_stepped, lp_graph=[t.clone() for t in eng._lp.tensors()])


@pytest.mark.parametrize("name,n_layer", [("tiny-test", None), ("7B", 2)])
def test_slot_engine_stepped_against_the_rules(name, n_layer):
    res = _slot_runs(name, n_layer)
    res["tally"].clean()
    assert res["tally"].draws == sum(min(b, STEPS + 1) for _, b, _, _ in res["reqs"].values())
    hist, state, adj, _ = res["stepped"]
    # the controls did something: the banned ids never came, and the runs of the three slots differ
    assert not np.isin(hist[1, :12], [100, 101]).any() and (state[1] & 0x7FFFFFFF).sum() == 11
    assert not np.isinf(R.decode(adj.reshape(-1), False)).any()


def test_captured_run_gives_the_stepped_runs_tokens():
    res = _slot_runs("tiny-test", None)
    (h0, s0, a0, _), (h1, s1, a1) = res["stepped"], res["graph"]
    for s, (_, budget, _, _) in res["reqs"].items():
        n = min(budget, STEPS + 1)
        assert h0[s, :n].tolist() == h1[s, :n].tolist(), s
    assert np.array_equal(s0, s1) and np.array_equal(a0, a1)


def test_logprobs_next_to_processors_are_the_models_own():
    res = _slot_runs("tiny-test", None)
    assert not res["stepped"][3], res["stepped"][3][:5]  # each token's logprob and alternates: the rule on the RAW logits
    for a, b in zip(res["lp_stepped"], res["lp_graph"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # ... and not the adjusted distribution's: slot 1's bias of +4 on token 3 would move every logprob of its row
    assert any(abs(float(x)) > 0 for x in res["lp_stepped"][0][1, :12])


def _run_graph(eng, reqs):
    _admit_all(eng, reqs)
    eng.run_steps(STEPS, use_graph=True, **KW)
    st = eng.read_state()
    assert st[SLOT_ACTIVE] == 0
    return {s: eng.read_history(s, st[SLOT_PRODUCED + s]) for s in reqs}


def test_a_request_without_controls_is_served_as_with_the_feature_off():
    # every row kept: with TEAL masks a step's sums are grouped by the union of the rows its sequences keep, so a neighbour that
    # draws other tokens can move a sequence's logits in the last place; with every row kept the union is every row whatever the
    # neighbours do, and only the processors could tell the runs apart
    m, ths = _model("tiny-test", None, 3, sparsity=0.0)
    eng = SlotDecodeEngine(m, ths, 3)
    plain = {s: (p, b, seed, {}) for s, (p, b, seed, _) in REQS3.items()}
    off = _run_graph(eng, plain)
    eng.set_logit_processors(True)
    on = _run_graph(eng, REQS3)  # request 2 (no controls) next to two requests with controls
    assert on[2] == off[2] and on[0] != off[0] and on[1] != off[1]
    assert _run_graph(eng, plain) == off  # everybody at identity parameters: nobody's tokens move
    moved = {0: REQS3[2], 1: REQS3[0], 2: REQS3[1]}  # the plain request in another slot, after the slot served a request with controls
    assert _run_graph(eng, moved)[0] == off[2]
    eng.set_logit_processors(False)
    assert _run_graph(eng, plain) == off
    with pytest.raises(RuntimeError, match="off"):
        eng.admit(0, [1, 2], 3, None, 1, **KW, repetition_penalty=1.2)
    with pytest.raises(RuntimeError, match="off"):
        eng.set_slot_processors(0, [1, 2])
    eng.admit(0, [1, 2], 3, None, 1, **KW, repetition_penalty=1.0)  # spelled-out identity needs nothing


def test_a_clamping_frequency_penalty_stops_every_repeat():
    m, ths = _model("tiny-test", None, 2)
    eng = SlotDecodeEngine(m, ths, 2)
    prompt, budget, seed = [5, 9, 300, 9, 17], MAX_SEQ - 6, 31  # 58 tokens from a vocabulary of 512, 50 of them eligible per draw
    eng.admit(0, prompt, budget, None, seed, **KW)
    eng.run_steps(budget - 1, use_graph=True, **KW)
    off = eng.read_history(0, eng.read_state()[SLOT_PRODUCED])
    assert len(off) == budget and len(set(off)) < len(off), "pick a seed whose plain run repeats a token"
    eng.set_logit_processors(True)
    eng.admit(0, prompt, budget, None, seed, **KW, frequency_penalty=1e6)  # one generation: -1e6, clamped to -65504
    eng.run_steps(budget - 1, use_graph=True, **KW)
    on = eng.read_history(0, eng.read_state()[SLOT_PRODUCED])
    assert len(on) == budget and len(set(on)) == len(on)
    assert on[0] == off[0]  # the first draw: nothing generated yet
    adj = R.decode(_bits(eng._proc.adj[0]), False)
    assert (adj[on[:-1]] == -65504.0).all() and np.isfinite(adj).all()
    for bad, msg in [(dict(repetition_penalty=0.0), "> 0"), (dict(frequency_penalty=float("inf")), "finite"), (dict(logit_bias={"512": 1.0}), "outside"),
                     (dict(logit_bias={"3": 1e6}), "not finite in"), (dict(presence_penalty=float("nan")), "finite")]:
        with pytest.raises(ValueError, match=msg):
            eng.admit(1, [1, 2], 3, None, 1, **KW, **bad)
    assert eng.read_state()[SLOT_ACTIVE] & 2 == 0  # refused before anything moved


def test_a_prefix_requests_prompt_bits_cover_the_prefix():
    m, ths = _model("tiny-test", None, 2)
    eng = SlotDecodeEngine(m, ths, 2)
    V = m.config.vocab_size
    pre, suffix = [400, 401, 402, 9, 400, 77, 78, 79, 80], [5, 9, 300]
    eng.register_prefix("sys", pre)
    eng.set_logit_processors(True)
    ctl = dict(repetition_penalty=1.5)
    eng.admit(1, suffix, 6, None, 41, **KW, prefix="sys", **ctl)
    torch.cuda.synchronize()
    want = R.prompt_state(V, pre + suffix)
    assert np.array_equal(eng._proc.state[1].cpu().numpy(), want) and int((want != 0).sum()) == len(set(pre + suffix))
    assert np.array_equal(_bits(eng._proc.adj[1]), _rule(_bits(eng.admit_logits.view(-1)), want, ctl))
    assert not eng._proc.state[0].any()
    tally = _Tally()
    tally.check_draw("admit", _bits(eng._proc.adj[1]), 41, 0, int(eng.history[1, 0]))
    assert not tally.draw


def test_decode_engine_adjusts_and_draws_by_the_rules():
    n = 10
    m, ths = _model("tiny-test", None, 1)
    V = m.config.vocab_size
    prompt = torch.tensor([5, 9, 300, 9, 17, 44], device=DEV, dtype=torch.int)
    ctl = dict(repetition_penalty=1.3, presence_penalty=0.25, frequency_penalty=0.5, logit_bias={"3": 3.0, "100": -100.0})
    with torch.no_grad():
        row = m(prompt.view(1, -1), torch.arange(6, device=DEV))[0, -1].clone()
        eng = DecodeEngine(m, ths)
        eng.manual_seed(5)
        first = eng.sample_first(row, **KW).clone()
        off = [int(first)] + eng.decode_n(first, 6, n, drawn=1, **KW).tolist()
        eng.set_logit_processors(True)
        tally = _Tally()
        # eagerly, one draw at a time
        eng.set_slot_processors(0, prompt.tolist(), **ctl)
        eng.manual_seed(5)
        first = eng.sample_first(row, **KW).clone()
        torch.cuda.synchronize()
        state = R.prompt_state(V, prompt.tolist())
        seed = int(eng.rng_state[0])
        tally.check_rows("first", _bits(eng._proc.adj[0]), _rule(_bits(row), state, ctl), eng._proc.state[0].cpu().numpy(), state)
        tally.check_draw("first", _bits(eng._proc.adj[0]), seed, 0, int(first))
        eng.tok_buf.copy_(first.view(1, 1))
        eng.pos_buf.fill_(6)
        toks = [int(first)]
        for i in range(n):
            fed = int(eng.tok_buf)
            eng._self_step(**KW)
            torch.cuda.synchronize()
            state = R.count(state, fed)
            tally.check_rows(i, _bits(eng._proc.adj[0]), _rule(_bits(eng.logits.view(-1)), state, ctl), eng._proc.state[0].cpu().numpy(), state)
            toks.append(int(eng.tok_buf))
            tally.check_draw(i, _bits(eng._proc.adj[0]), seed, i + 1, toks[-1])
        tally.clean()
        assert toks != off and 100 not in toks
        # the same sample through generate()'s calls and the captured step
        eng.set_slot_processors(0, prompt.tolist(), **ctl)
        eng.manual_seed(5)
        first2 = eng.sample_first(row, **KW).clone()
        graph = [int(first2)] + eng.decode_n(first2, 6, n, drawn=1, **KW).tolist()
        assert graph == toks and np.array_equal(eng._proc.state[0].cpu().numpy(), state)
        # decode_n(prompt_tokens=...): the state starts over, the given first token is counted by the first step
        eng.manual_seed(9)
        a = eng.decode_n(first, 6, n, prompt_tokens=prompt.tolist(), **KW).tolist()
        want = R.prompt_state(V, prompt.tolist())
        for t in [int(first)] + a[:-1]:
            want = R.count(want, t)
        assert np.array_equal(eng._proc.state[0].cpu().numpy(), want)
        eng.manual_seed(9)
        assert eng.decode_n(first, 6, n, prompt_tokens=prompt.tolist(), **KW).tolist() == a
        eng.set_logit_processors(False)
        eng.manual_seed(5)
        first = eng.sample_first(row, **KW).clone()
        assert [int(first)] + eng.decode_n(first, 6, n, drawn=1, **KW).tolist() == off
    eng.reduce = lambda t: t  # what tp.apply_tp leaves on a sharded model's engine
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        eng.set_logit_processors(True)


def test_batched_engine_adjusts_and_draws_by_the_rules():
    B, n = 3, 8
    m, ths = _model("tiny-test", None, B)
    V = m.config.vocab_size
    eng = BatchedDecodeEngine(m, ths, B)
    first = torch.tensor([5, 9, 300], device=DEV, dtype=torch.int32)
    prompts = [[1, 2, 3], [9, 9], [300, 4, 5, 6]]
    ctls = [dict(frequency_penalty=0.7), dict(), dict(repetition_penalty=0.8, logit_bias={"7": 200.0})]
    eng.manual_seed(3)
    off = eng.decode_n(first, 0, n, **KW)
    eng.set_logit_processors(True)
    for b in range(B):
        eng.set_slot_processors(b, prompts[b], **ctls[b])
    eng.tok_buf[:B].copy_(first)
    eng.pos_buf[:B].fill_(0)
    eng.rng_state.copy_(torch.tensor([[3 + b, 0] for b in range(B)], dtype=torch.int64))
    state = np.stack([R.prompt_state(V, p) for p in prompts])
    tally = _Tally()
    for i in range(n):
        fed = eng.tok_buf[:B].tolist()
        eng._self_step(**KW)
        torch.cuda.synchronize()
        raw = _bits(eng.logits)
        for b in range(B):
            state[b] = R.count(state[b], fed[b])
        want = np.stack([_rule(raw[b], state[b], ctls[b]) for b in range(B)])
        tally.check_rows(i, _bits(eng._proc.adj), want, eng._proc.state.cpu().numpy(), state)
        for b in range(B):
            tally.check_draw((i, b), want[b], 3 + b, i, int(eng.tok_buf[b]))
    tally.clean()
    eager = eng.history[:, :n].clone()
    assert eager[2].tolist() == [7] * n and off[2].tolist() != [7] * n  # a bias far above every logit: that token
    eng.manual_seed(3)
    graph = eng.decode_n(first, 0, n, prompt_tokens=prompts, **KW)
    assert torch.equal(graph, eager) and np.array_equal(eng._proc.state.cpu().numpy(), state)
    eng.set_logit_processors(False)
    eng.manual_seed(3)
    assert torch.equal(eng.decode_n(first, 0, n, **KW), off)


class _Count:
    """a library handle that records which entry points are called"""

    def __init__(self, L, calls):
        self._L, self._calls = L, calls

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("teal_"):
            return f

        def call(*a):
            self._calls.append(name)
            return f(*a)
        return call


def test_with_the_feature_off_a_step_launches_what_it_launched_before():
    B = 3
    m, ths = _model("tiny-test", None, B)
    eng = SlotDecodeEngine(m, ths, B)
    _admit_all(eng, {s: (p, b, seed, {}) for s, (p, b, seed, _) in REQS3.items()})

    def step_calls():
        calls, keep = [], eng.L
        eng.L = _Count(keep, calls)
        if eng._proc is not None:
            eng._proc.L = _Count(keep, calls)
        try:
            eng._self_step(**KW)
        finally:
            eng.L = keep
        return calls

    fresh = step_calls()
    n_layers = len(m.layers)
    # embedding rows; per layer qkv, attention, wo, resid, gate|up, down, resid; lm_head and its rounding; B samplers; retire
    assert len(fresh) == 1 + 7 * n_layers + 2 + B + 1 and "teal_logit_adjust" not in fresh
    eng.set_logit_processors(True)
    on = step_calls()
    assert eng.adj_logits.shape == eng.logits.shape and eng.adj_logits.data_ptr() != eng.logits.data_ptr()
    assert eng.lp_state.dtype == torch.int32 and eng.lp_params[0].tolist() == [1.0, 0.0, 0.0, 0.0] and not eng.lp_bias.any()
    assert len(on) == len(fresh) + 1 and on.count("teal_logit_adjust") == 1
    assert on.index("teal_logit_adjust") == on.index("teal_sample_topk_slot") - 1  # between the logits and the first sampler
    eng.set_logit_processors(False)
    assert step_calls() == fresh and eng._proc is None and eng.adj_logits is None and eng.lp_state is None


def _calls_of(eng, step):
    """the entry points `step` calls through the engine's library handles"""
    calls, keep = [], eng.L
    eng.L = _Count(keep, calls)
    if eng._proc is not None:
        eng._proc.L = _Count(keep, calls)
    try:
        step()
    finally:
        eng.L = keep
    return calls


def test_the_non_slot_engines_launch_what_they_launched_with_the_feature_off():
    m, ths = _model("tiny-test", None, 1)
    n_layers = len(m.layers)
    eng = DecodeEngine(m, ths)
    eng.tok_buf.fill_(5)
    eng.pos_buf.fill_(3)
    step = lambda: eng._self_step(**KW)  # noqa: E731
    fresh = _calls_of(eng, step)
    # per layer qkv, attention, wo, gate|up, down; lm_head; the sampler
    assert fresh.count("teal_fused_gemv") == 4 * n_layers + 1 and len(fresh) == 5 * n_layers + 2 and "teal_logit_adjust" not in fresh
    eng.set_logit_processors(True)
    on = _calls_of(eng, step)
    assert len(on) == len(fresh) + 1 and on.index("teal_logit_adjust") == on.index("teal_sample_topk_ws") - 1
    eng.set_logit_processors(False)
    assert _calls_of(eng, step) == fresh and eng.adj_logits is None
    B = 3
    mb, thb = _model("tiny-test", None, B)
    engb = BatchedDecodeEngine(mb, thb, B)
    stepb = lambda: engb._self_step(**KW)  # noqa: E731
    fresh = _calls_of(engb, stepb)
    assert len(fresh) == 1 + 7 * n_layers + 2 + B and "teal_logit_adjust" not in fresh
    engb.set_logit_processors(True)
    on = _calls_of(engb, stepb)
    assert len(on) == len(fresh) + 1 and on.index("teal_logit_adjust") == on.index("teal_sample_topk_ws") - 1
    engb.set_logit_processors(False)
    assert _calls_of(engb, stepb) == fresh


def _main(*extra, new=12):
    return G.main(G.build_parser().parse_args(["--device", "cuda", "--synthetic", "tiny-test", "--sparsity", "0.5", "--num_samples", "1",
                                               "--max_new_tokens", str(new), *extra]))


def test_generate_requests_end_to_end_with_mixed_controls(tmp_path):
    f = tmp_path / "reqs.jsonl"
    f.write_text('{"tokens": [1, 2, 3]}\n'
                 '{"tokens": [4], "max_new_tokens": 30, "frequency_penalty": 1000000}\n'
                 '{"tokens": [5, 6, 7, 8, 9], "max_new_tokens": 9, "logit_bias": {"77": 200}}\n'
                 '{"tokens": [10, 11], "max_new_tokens": 20, "repetition_penalty": 1.0, "logit_bias": {"1": -100, "2": -100}}\n'
                 '{"tokens": [12], "max_new_tokens": 5, "presence_penalty": 0.5, "repetition_penalty": 1.3}\n')
    res = _main("--compile", "--requests", str(f), "--batch_size", "2", "--repetition_penalty", "1.1", "--logprobs", "0")
    seqs = res["sequences"]
    assert [len(s) for s in seqs] == [12, 30, 9, 20, 5]
    assert len(set(seqs[1])) == 30            # a clamping frequency penalty: no repeats
    assert seqs[2] == [77] * 9                # a bias far above every logit: that token
    assert not {1, 2} & set(seqs[3])          # banned tokens
    assert [len(x) for x in res["logprobs"]] == [len(s) for s in seqs] and all(v <= 0.0 for x in res["logprobs"] for v in x)
    assert res["logprobs"][2][0] < -1.0       # the forced token's logprob is the MODEL's: unlikely, not ~0
    # the single-sequence and the --batch_size engine paths take the flags too
    # (50 draws from the 50 most likely of 512 tokens: the plain sample repeats itself, the penalised one cannot)
    plain, pen = _main("--compile", new=50), _main("--compile", "--frequency_penalty", "1000000", new=50)
    old, new = plain["sequences"][0][6:], pen["sequences"][0][6:]
    assert len(old) == len(new) == 50 and len(set(old)) < 50 and len(set(new)) == 50
    plain, bat = _main("--compile", "--batch_size", "3", new=50), _main("--compile", "--batch_size", "3", "--frequency_penalty", "1000000", new=50)
    for a, b in zip(plain["sequences"][0], bat["sequences"][0]):
        # (the first new token comes from the prompt pass's torch sampler; it is counted as generated like the rest)
        assert len(b[6:]) == 50 and len(set(b[6:])) == 50 and len(set(a[6:])) < 50
