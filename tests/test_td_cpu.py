"""The TD(lambda) arithmetic (narde_rules.h "TD(lambda)": what k_td_trace
runs) on the CPU, through a test-only host build that takes a wave's lanes in
turn (tests/hostcheck/hostcheck_td.cpp), on the golden states and their
mover-flipped copies.

Reference: td_ref's explicit per-sample formulas in float64 on O.tesauro198
rows.  Tolerance: 8 x E, E = max |the same formulas in float32 - float64| per
compared array (floored at one float32 ulp of its largest magnitude) -- the
reference's own rounding, never the code under test's.  make_net's scaling
makes a dropped column move a gradient element from |d_h| ~ 1e-2 to zero.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import td_ref as T
from conftest import ROOT
from test_afterstates_cpu import golden_states
from test_value_cpu import NETS, make_net

torch = pytest.importorskip("torch")

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
CHUNK = 1001
DECAYS = (0.0, 0.7, 1.0)


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_td.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_td.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    lib.hc_td_row_floats.restype = ctypes.c_int64
    return lib


@pytest.fixture(scope="module")
def states():
    """(board, off, player, feat): the golden states, then the same with the
    other side to move."""
    board, off, _, player, _ = golden_states()
    assert len(player) == 4004
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off = c(np.concatenate([board, board]), np.int8), c(np.concatenate([off, off]), np.uint8)
    player = c(np.concatenate([player, -np.asarray(player)]), np.int8)
    return board, off, player, O.tesauro198(board, off, player)


def host_trace(hc, net, board, off, player, decay, trace):
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    n = len(player)
    w1t = np.ascontiguousarray(net.l1.weight.detach().numpy().T, dtype=np.float32)
    b1 = np.ascontiguousarray(net.l1.bias.detach().numpy(), dtype=np.float32)
    w2 = np.ascontiguousarray(net.l2.weight.detach().numpy().reshape(-1), dtype=np.float32)
    b2 = np.ascontiguousarray(net.l2.bias.detach().numpy(), dtype=np.float32)
    v, black = np.full(n, np.nan, np.float32), np.full(n, 9, np.uint8)
    cols = np.full((n, 198), 9, np.uint8)
    assert trace.dtype == np.float32 and trace.flags.c_contiguous and trace.shape[0] == n
    hc.hc_td_trace(ctypes.c_int64(n), P(board), P(off), P(player), P(w1t), ctypes.c_int64(w1t.shape[1]), P(b1), P(w2),
                   P(b2), net.hidden, HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act], ctypes.c_float(decay),
                   P(trace), ctypes.c_int64(trace.shape[1]), P(v), P(black), P(cols))
    return v, black, cols


def test_layout_constants(hc):
    from gym_narde import _lib

    assert hc.hc_td_slab() == _lib.TD_SLAB
    for h in (1, 80, 128):
        assert hc.hc_td_row_floats(h) == T.row_floats(h) == 200 * h + 1


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_value_gradient_and_trace_rows(hc, states, spec):
    board, off, player, feat = states
    net = make_net(*spec)
    H = net.hidden
    Pn = T.row_floats(H)
    pad = 3  # floats past the row: never touched
    p32, p64 = T.params_of(net, torch.float32), T.params_of(net, torch.float64)
    bv, bg = T.Bound(f"v {spec[:3]}"), T.Bound(f"grad {spec[:3]}")
    bt = {d: T.Bound(f"trace decay {d} {spec[:3]}") for d in DECAYS}
    rng = np.random.default_rng(7)
    spread = 0.0
    for i0 in range(0, len(player), CHUNK):
        sl = slice(i0, i0 + CHUNK)
        x = torch.from_numpy(feat[sl])
        v32, g32 = T.value_and_grad(p32, x, net.hidden_act, net.out_act)
        v64, g64 = T.value_and_grad(p64, x.double(), net.hidden_act, net.out_act)
        n = x.shape[0]
        # decay 0 over a NaN-filled row: the gradient itself, nothing read
        row = np.full((n, Pn + pad), np.nan, np.float32)
        v, black, cols = host_trace(hc, net, board[sl], off[sl], player[sl], 0.0, row)
        assert np.isnan(row[:, Pn:]).all() and not np.isnan(row[:, :Pn]).any()
        assert np.array_equal(black, (player[sl] == -1).astype(np.uint8))
        bv.add(v, v32.numpy(), v64.numpy())
        grad = row[:, :Pn].copy()
        bg.add(grad, g32.numpy(), g64.numpy())
        bt[0.0].add(grad, g32.numpy(), g64.numpy())
        # the W1 block is non-zero exactly on the record's own columns
        assert np.array_equal(cols, (feat[sl] != 0).astype(np.uint8))
        w1 = grad[:, :198 * H].reshape(n, 198, H)
        assert (w1[cols == 0] == 0).all()
        d = grad[:, 198 * H:199 * H]
        live = np.broadcast_to((d != 0)[:, None, :], w1.shape)[cols == 1]
        assert ((w1[cols == 1] != 0) == live).all()  # zero there only where d_h itself is (a relu unit that is off)
        spread = max(spread, float(np.abs(d).max()))
        for decay in DECAYS[1:]:
            prev = rng.standard_normal((n, Pn + pad)).astype(np.float32)
            row = prev.copy()
            host_trace(hc, net, board[sl], off[sl], player[sl], decay, row)
            assert np.array_equal(row[:, Pn:], prev[:, Pn:])
            t32 = torch.tensor(decay, dtype=torch.float32) * torch.from_numpy(prev[:, :Pn]) + g32
            t64 = decay * torch.from_numpy(prev[:, :Pn]).double() + g64
            bt[decay].add(row[:, :Pn], t32.numpy(), t64.numpy())
    assert bv.e > 0 and bg.e > 0
    assert spread > 1e3 * T.TOL_FACTOR * bg.e or H == 1  # a dropped column would show
    for b in (bv, bg, *bt.values()):
        b.check()


def test_td_error_rule(hc):
    rng = np.random.default_rng(3)
    n = 4096
    term = (rng.random(n) < 0.3).astype(np.uint8)
    trunc = (rng.random(n) < 0.3).astype(np.uint8)
    reward = np.where(term, rng.integers(1, 3, n), 0).astype(np.int32)
    black = rng.integers(0, 2, n).astype(np.uint8)
    v, vn = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    got = np.full(n, np.nan, np.float32)
    gamma = np.float32(0.9)
    hc.hc_td_delta(ctypes.c_int64(n), P(term), P(trunc), P(reward), P(black), ctypes.c_float(gamma), P(vn), P(v),
                   P(got))
    t = torch.from_numpy
    want = T.td_targets(t(v), t(vn), t(reward), t(black), t(term), t(trunc), torch.tensor(gamma))
    assert np.array_equal(got, want.numpy())  # one multiply and one subtract: exact
    assert (got[(trunc == 1) & (term == 0)] == 0).all()
