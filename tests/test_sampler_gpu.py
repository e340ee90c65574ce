"""GPU: every kernel and entry point of the fused top-k sampler (teal_sampler.hip) against the host model of its draw
(tests/sampler_rule.py) — not against each other.

  teal_sample_topk        no workspace: the single-workgroup kernels (window NV = 4 / NV = 16, generic radix)
  teal_sample_topk_ws     a prepared workspace: the multi-workgroup kernel where sample_launch allows it
  teal_sample_topk_slot   the *_slot_kernel forms, with and without a workspace; bit set -> the model's token, bit clear -> nothing moves

Which kernel a vocabulary size reaches is written next to it in sampler_cases.VOCABS; the inputs (laws, top_k, temperatures,
seeds) are sampler_cases.cases(V), the same bits tests/test_sampler_rule.py checks the model's `open` share on.  Where the model
says a draw is not open the token must be the model's; where it is open, the model's token or its runner-up; more than 1 % open
draws in a case fail it.  Tokens, history, rng_state and pos are read once per test, after the last launch.
"""
import time

import numpy as np
import pytest
import torch

import sampler_cases as C
import sampler_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77      # what history, token slots and positions hold before a launch
POS0 = 11
SLOT = 5        # the bit teal_sample_topk_slot looks at


def _lib_rt():
    from teal_amd import _lib, runtime
    L = _lib.load()
    runtime.init()
    return L, runtime


def _upload(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.view(np.int16).copy()).to(DEV)


def _launcher(L, runtime, entry, ws, active):
    """entry -> f(logits_ptr, V, code, top_k, T, state_ptr, tok_ptr, pos_ptr, hist_ptr, hist_len) on the current stream"""
    wp, wb = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
    ap = active.data_ptr() if active is not None else None
    if entry == "plain":
        return lambda *a: L.teal_sample_topk(*a, runtime.stream_ptr())
    if entry == "ws":
        return lambda *a: L.teal_sample_topk_ws(*a, wp, wb, runtime.stream_ptr())
    if entry == "slot_ws":
        return lambda *a: L.teal_sample_topk_slot(*a, wp, wb, ap, SLOT, runtime.stream_ptr())
    if entry == "slot_plain":
        return lambda *a: L.teal_sample_topk_slot(*a, None, 0, ap, SLOT, runtime.stream_ptr())
    raise KeyError(entry)


def _check(label, got, model):
    tok, ru, op = model
    assert op.mean() <= 0.01, (label, "open draws", float(op.mean()))
    bad = (got != tok) & ~(op & (got == ru))
    assert not bad.any(), (label, "draws", np.flatnonzero(bad)[:6].tolist(), "kernel", got[bad][:6].tolist(), "model", tok[bad][:6].tolist())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", list(C.VOCABS))
def test_every_entry_point_draws_the_models_tokens(V, dtype):
    L, runtime = _lib_rt()
    bf16, code = dtype == torch.bfloat16, runtime.dtype_code(dtype)
    ws = runtime.new_workspace(64, 64)
    active = torch.tensor([(1 << SLOT) | 1], dtype=torch.int32, device=DEV)
    # without a workspace the slot entry point reaches another kernel than with one only where the multi-workgroup kernel applies
    entries = ("plain", "ws", "slot_ws") + (("slot_plain",) if V > 8192 else ())
    fns = {e: _launcher(L, runtime, e, ws, active) for e in entries}
    cases = C.cases(V)
    runs = [(ci, bi, e) for ci in range(len(cases)) for bi in range(2) for e in entries]
    NH = C.N_MAIN
    state_h = np.empty((len(runs), 2), dtype=np.int64)
    for r, (ci, bi, _) in enumerate(runs):
        state_h[r] = C.blocks(cases[ci][3])[bi][:2]
    state = torch.from_numpy(state_h).to(DEV)
    tok = torch.full((len(runs), NH), SENT, dtype=torch.int32, device=DEV)
    hist = torch.full((len(runs), NH + 1), SENT, dtype=torch.int32, device=DEV)
    pos = torch.full((len(runs),), POS0, dtype=torch.int32, device=DEV)
    logits = {law: _upload(C.logits_bits(law, V, bf16)) for law in {c[0] for c in cases}}
    sp, tp, hp, pp = state.data_ptr(), tok.data_ptr(), hist.data_ptr(), pos.data_ptr()
    t0 = time.perf_counter()
    for r, (ci, bi, e) in enumerate(runs):
        law, top_k, T, seed = cases[ci]
        lp, fn = logits[law].data_ptr(), fns[e]
        for j in range(C.blocks(seed)[bi][2]):
            rc = fn(lp, V, code, top_k, T, sp + 16 * r, tp + 4 * (r * NH + j), pp + 4 * r, hp + 4 * r * (NH + 1), NH)
            assert rc == 0, (rc, cases[ci], e)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    tok_h, hist_h, state_h2, pos_h = tok.cpu().numpy(), hist.cpu().numpy(), state.cpu().numpy(), pos.cpu().numpy()
    assert int(active.item()) == (1 << SLOT) | 1
    model = {}
    share = 0.0
    for r, (ci, bi, e) in enumerate(runs):
        law, top_k, T, seed = cases[ci]
        s, c0, n = C.blocks(seed)[bi]
        if (ci, bi) not in model:
            model[ci, bi] = R.draws(C.logits_bits(law, V, bf16), bf16, top_k, T, s, c0, n)
            share = max(share, float(model[ci, bi][2].mean()))
        label = (V, "bf16" if bf16 else "fp16", law, top_k, T, f"seed {s} ctr {c0}", e)
        got = tok_h[r, :n]
        assert (tok_h[r, n:] == SENT).all(), label
        _check(label, got, model[ci, bi])
        # the bookkeeping: seed kept, counter + n, position + n, history filed under the draw counter where it is below history_len
        assert state_h2[r].tolist() == [s, c0 + n], (label, state_h2[r].tolist())
        assert pos_h[r] == POS0 + n, (label, int(pos_h[r]))
        want_hist = np.full(NH + 1, SENT, dtype=np.int32)
        if c0 == 0:
            want_hist[:n] = got
        assert np.array_equal(hist_h[r], want_hist), (label, hist_h[r].tolist())
    print(f"V={V} {'bf16' if bf16 else 'fp16'}: {len(cases)} cases x {len(entries)} entry points, {int(sum(C.blocks(cases[ci][3])[bi][2] for ci, bi, _ in runs))} "
          f"launches in {t1 - t0:.2f} s, model {time.perf_counter() - t1:.2f} s, largest share of open draws {share:.4f}")


# (vocab, workspace, top_k, law) -> the slot kernel the call reaches
SLOT_CASES = [(8, True, 2, "normal"),          # window_slot NV = 4
              (1000, True, 20, "normal"),      # generic slot kernel
              (8192, False, 20, "flat"),       # window_slot NV = 4, full
              (8200, True, 20, "normal"),      # multi_slot, 2 workgroups: every workgroup must take the same exit
              (32776, False, 20, "normal"),    # window_slot NV = 16
              (131072, True, 513, "fewvals"),  # multi_slot, 16 workgroups, candidate overflow -> the generic body
              (131072, True, 0, "normal"),     # no filter: window_slot NV = 16 although a workspace is there
              (131080, True, 20, "tail")]      # generic slot kernel past every limit


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_slot_bit_clear_moves_nothing_and_bit_set_draws(dtype):
    L, runtime = _lib_rt()
    bf16, code = dtype == torch.bfloat16, runtime.dtype_code(dtype)
    ws = runtime.new_workspace(64, 64)
    off = torch.tensor([~(1 << SLOT) & 0x7FFFFFFF], dtype=torch.int32, device=DEV)  # every bit but the slot's
    on = torch.tensor([1 << SLOT], dtype=torch.int32, device=DEV)
    n = 4
    keep = []
    for V, use_ws, top_k, law in SLOT_CASES:
        bits = C.logits_bits(law, V, bf16)
        lg = _upload(bits)
        state = torch.tensor([C.SEED, 2], dtype=torch.int64, device=DEV)
        tok = torch.full((n + 1,), SENT, dtype=torch.int32, device=DEV)
        hist = torch.full((8,), SENT, dtype=torch.int32, device=DEV)
        pos = torch.full((1,), POS0, dtype=torch.int32, device=DEV)
        wp, wb = (ws.data_ptr(), ws.numel() * 4) if use_ws else (None, 0)
        for j in range(n):  # bit clear
            assert L.teal_sample_topk_slot(lg.data_ptr(), V, code, top_k, 0.8, state.data_ptr(), tok.data_ptr() + 4 * j, pos.data_ptr(),
                                           hist.data_ptr(), 8, wp, wb, off.data_ptr(), SLOT, runtime.stream_ptr()) == 0
        snap = [t.clone() for t in (state, tok, hist, pos)]
        for j in range(n):  # bit set: draws 2 .. 5 of the stream (a skipped multi-workgroup launch left its arrival ticket armed)
            assert L.teal_sample_topk_slot(lg.data_ptr(), V, code, top_k, 0.8, state.data_ptr(), tok.data_ptr() + 4 * j, pos.data_ptr(),
                                           hist.data_ptr(), 8, wp, wb, on.data_ptr(), SLOT, runtime.stream_ptr()) == 0
        keep.append((V, use_ws, top_k, law, bits, snap, state, tok, hist, pos, lg))
    torch.cuda.synchronize()
    for V, use_ws, top_k, law, bits, snap, state, tok, hist, pos, _ in keep:
        label = (V, use_ws, top_k, law)
        assert snap[0].tolist() == [C.SEED, 2] and (snap[1] == SENT).all() and (snap[2] == SENT).all() and snap[3].tolist() == [POS0], label
        got = tok.cpu().numpy()
        model = R.draws(bits, bf16, top_k, 0.8, C.SEED, 2, n)
        _check(label, got[:n], model)
        assert got[n] == SENT and state.tolist() == [C.SEED, 2 + n] and pos.tolist() == [POS0 + n], label
        assert hist.tolist() == [SENT, SENT] + got[:n].tolist() + [SENT, SENT], label
    for bad_slot in (-1, 32):
        assert L.teal_sample_topk_slot(lg.data_ptr(), V, code, top_k, 0.8, state.data_ptr(), tok.data_ptr(), pos.data_ptr(), hist.data_ptr(), 8,
                                       None, 0, on.data_ptr(), bad_slot, runtime.stream_ptr()) < 0
    assert L.teal_sample_topk_slot(lg.data_ptr(), V, code, top_k, 0.8, state.data_ptr(), tok.data_ptr(), pos.data_ptr(), hist.data_ptr(), 8,
                                   None, 0, None, SLOT, runtime.stream_ptr()) < 0


# (vocab, entry, top_k, law) -> the body whose history guard is exercised
GUARD_CASES = [(1000, "plain", 20, "normal"),       # generic
               (4096, "plain", 20, "normal"),       # window NV = 4
               (32776, "plain", 20, "normal"),      # window NV = 16
               (32776, "ws", 20, "normal"),         # multi-workgroup, stage B
               (32768, "ws", 20, "fewvals"),        # multi-workgroup, candidate overflow -> the generic body
               (8200, "slot_ws", 20, "flat")]       # multi-workgroup slot form


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_history_guard(dtype):
    """history_len = 4: draws 4 onward must not write history (element 4 keeps its sentinel) while the counter still advances"""
    L, runtime = _lib_rt()
    bf16, code = dtype == torch.bfloat16, runtime.dtype_code(dtype)
    ws = runtime.new_workspace(64, 64)
    active = torch.tensor([1 << SLOT], dtype=torch.int32, device=DEV)
    n, keep = 8, []
    for V, entry, top_k, law in GUARD_CASES:
        fn = _launcher(L, runtime, entry, ws, active)
        bits = C.logits_bits(law, V, bf16)
        lg = _upload(bits)
        state = torch.tensor([C.SEED, 0], dtype=torch.int64, device=DEV)
        tok = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
        hist = torch.full((5,), SENT, dtype=torch.int32, device=DEV)
        pos = torch.full((1,), POS0, dtype=torch.int32, device=DEV)
        for j in range(n):
            assert fn(lg.data_ptr(), V, code, top_k, 1.0, state.data_ptr(), tok.data_ptr() + 4 * j, pos.data_ptr(), hist.data_ptr(), 4) == 0
        keep.append((V, entry, top_k, law, bits, state, tok, hist, pos, lg))
    torch.cuda.synchronize()
    for V, entry, top_k, law, bits, state, tok, hist, pos, _ in keep:
        label = (V, entry, top_k, law)
        got = tok.cpu().numpy()
        _check(label, got, R.draws(bits, bf16, top_k, 1.0, C.SEED, 0, n))
        assert hist.tolist() == got[:4].tolist() + [SENT], (label, hist.tolist())
        assert state.tolist() == [C.SEED, n] and pos.tolist() == [POS0 + n], label


@pytest.mark.parametrize("V,use_ws,top_k,law", [(4096, False, 20, "normal"),     # window NV = 4
                                                (32768, True, 20, "normal"),      # multi-workgroup: the ticket re-arms between replays
                                                (32001, True, 513, "flat")])      # generic
def test_graph_replay_draws_the_models_tokens(V, use_ws, top_k, law):
    """one captured launch, 16 replays: the draw counter lives on the device, so the replays are draws 0 .. 15"""
    L, runtime = _lib_rt()
    bf16, code, n = True, 1, 16
    ws = runtime.new_workspace(64, 64)
    bits = C.logits_bits(law, V, bf16)
    lg = _upload(bits)
    state = torch.tensor([C.SEED, 0], dtype=torch.int64, device=DEV)
    tok = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
    hist = torch.full((n + 1,), SENT, dtype=torch.int32, device=DEV)
    pos = torch.full((1,), POS0, dtype=torch.int32, device=DEV)
    fn = _launcher(L, runtime, "ws" if use_ws else "plain", ws, None)

    def step():
        assert fn(lg.data_ptr(), V, code, top_k, 0.8, state.data_ptr(), tok.data_ptr(), pos.data_ptr(), hist.data_ptr(), n) == 0

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture, then the state it moved is put back
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    state.copy_(torch.tensor([C.SEED, 0], dtype=torch.int64))
    hist.fill_(SENT)
    pos.fill_(POS0)
    g = torch.cuda.CUDAGraph()
    with runtime.graph_capture(g):
        step()
    for _ in range(n):
        g.replay()
    torch.cuda.synchronize()
    got = hist.cpu().numpy()
    _check((V, use_ws, top_k, law, "graph"), got[:n], R.draws(bits, bf16, top_k, 0.8, C.SEED, 0, n))
    assert got[n] == SENT and state.tolist() == [C.SEED, n] and pos.tolist() == [POS0 + n] and int(tok) == got[n - 1]
