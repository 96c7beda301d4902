"""The windowed TD(lambda) update (narde_rules.h "windowed TD(lambda)": what
narde_value_td_window's kernels run) on the CPU, through a test-only host
build that runs the passes serially in the kernels' summation order
(tests/hostcheck/hostcheck_td_window.cpp), on windows cut from the golden
states and their mover-flipped copies with synthetic reward / terminated /
truncated flags.

Reference: the semantics as narde.h states them, in torch float64 --
td_ref.value_and_grad for v and the gradient rows, td_ref.td_targets for
delta, the backward recursion for G, theta + alpha sum G grad.  Tolerance:
8 x E, E = max |the same formulas in float32 - float64| per compared array
(floored at one float32 ulp of its largest magnitude), td_ref's rule.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import td_ref as T
from conftest import ROOT
from test_afterstates_cpu import golden_states
from test_value_cpu import make_net

torch = pytest.importorskip("torch")

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
NETS = [(80, "sigmoid", "sigmoid", 1), (128, "tanh", "none", 2), (1, "relu", "none", 3), (65, "relu", "tanh", 4)]
SHAPES = [(K, B) for K in (1, 2, 7) for B in (1, 65)]
ALPHA, GAMMA = 0.05, 0.9


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_td_window.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_td_window.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    lib.hc_tdw_scratch_floats.restype = ctypes.c_int64
    lib.hc_tdw_scratch_macro.restype = ctypes.c_int64
    return lib


@pytest.fixture(scope="module")
def states():
    """(board, off, player, feat): the golden states interleaved with their
    mover-flipped copies, so that every window holds both colours."""
    board, off, _, player, _ = golden_states()
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    n = len(player)
    flip = np.where(np.arange(n) % 3 == 1, -1, 1).astype(np.int8)
    board, off, player = c(board, np.int8), c(off, np.uint8), c(np.asarray(player) * flip, np.int8)
    return board, off, player, O.tesauro198(board, off, player)


def window(states, K, B, start):
    """Samples k B + e of a window: (K + 1) B consecutive states from `start`."""
    board, off, player, feat = states
    sl = slice(start, start + (K + 1) * B)
    assert sl.stop <= len(player)
    return board[sl], off[sl], player[sl], feat[sl]


def flags(K, B, player):
    """Synthetic (reward, terminated, truncated) [K][B]: sparse random
    endings, then the placed ones the issue lists (where the shape has room)."""
    rng = np.random.default_rng(100 * K + B)
    term = (rng.random((K, B)) < 0.12).astype(np.uint8)
    trunc = ((rng.random((K, B)) < 0.08) & (term == 0)).astype(np.uint8)
    black = (player[:K * B].reshape(K, B) == -1)
    if B == 1:
        term[0, 0], trunc[0, 0] = 1, 0  # an ending at k = 0 ...
        if K > 1:
            term[K - 1, 0], trunc[K - 1, 0] = 0, 1  # ... and one at K - 1: two in one env
    else:
        eb, ew = int(np.argmax(black[0])), int(np.argmax(~black[0]))
        term[0, eb], trunc[0, eb] = 1, 0  # a terminal ply by black at k = 0
        term[0, ew], trunc[0, ew] = 1, 0  # and one by white
        et = next(e for e in range(B) if e not in (eb, ew))
        term[K - 1, et], trunc[K - 1, et] = 0, 1  # a truncation at k = K - 1
        if K > 1:
            term[K - 1, eb] = 1  # two endings in one env
            trunc[K - 1, eb] = 0
    reward = np.where(term == 1, 1 + (np.arange(K * B).reshape(K, B) % 2), 0).astype(np.int32)
    return reward, term, trunc


def check_flags(K, B, player, reward, term, trunc):
    black = (player[:K * B].reshape(K, B) == -1)
    ended = (term | trunc).astype(bool)
    assert ended[0].any() and ended[K - 1].any()
    if K * B >= 65:
        assert (term.astype(bool) & black).any() and (term.astype(bool) & ~black).any()
        assert set(reward[term == 1]) == {1, 2} and (reward[term == 0] == 0).all()
        assert (trunc == 1).any()
    if K > 1:
        assert (ended.sum(0) >= 2).any()


def host_window(hc, net, board, off, player, reward, term, trunc, K, B, lam):
    """(v, delta, G, theta): the host passes on a copy of the net's weights."""
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    H = net.hidden
    w1t = np.ascontiguousarray(net.l1.weight.detach().numpy().T, dtype=np.float32).copy()
    b1 = net.l1.bias.detach().numpy().astype(np.float32).copy()
    w2 = net.l2.weight.detach().numpy().reshape(-1).astype(np.float32).copy()
    b2 = net.l2.bias.detach().numpy().astype(np.float32).copy()
    v = np.full((K + 1) * B, np.nan, np.float32)
    delta, G = np.full(K * B, np.nan, np.float32), np.full(K * B, np.nan, np.float32)
    c = np.ascontiguousarray
    hc.hc_td_window(K, ctypes.c_int64(B), P(board), P(off), P(player), P(c(reward)), P(c(term)), P(c(trunc)), P(w1t),
                    ctypes.c_int64(H), P(b1), P(w2), P(b2), H, HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act],
                    ctypes.c_float(ALPHA), ctypes.c_float(lam), ctypes.c_float(GAMMA), P(v), P(delta), P(G))
    theta = np.concatenate([w1t.reshape(-1), b1, w2, b2])
    return v.reshape(K + 1, B), delta.reshape(K, B), G.reshape(K, B), theta


def reference(params, feat, player, reward, term, trunc, K, B, lam, hidden_act, out_act):
    """narde.h's semantics in params' dtype: (v, delta, G, theta)."""
    dt = params[0].dtype
    x = torch.from_numpy(feat).to(dt)
    v, grad = T.value_and_grad(params, x, hidden_act, out_act)
    v = v.reshape(K + 1, B)
    black = torch.from_numpy((player[:K * B] == -1).reshape(K, B))
    tm, tr = torch.from_numpy(term), torch.from_numpy(trunc)
    gamma = torch.tensor(GAMMA, dtype=dt)
    delta = T.td_targets(v[:K], v[1:], torch.from_numpy(reward), black, tm, tr, gamma)
    c = torch.where((tm | tr).bool(), torch.zeros((), dtype=dt), gamma * torch.tensor(lam, dtype=dt))
    G = torch.zeros_like(delta)
    nxt = torch.zeros(B, dtype=dt)
    for k in range(K - 1, -1, -1):
        nxt = delta[k] + c[k] * nxt
        G[k] = nxt
    theta = T.theta_row(params) + torch.tensor(ALPHA, dtype=dt) * (G.reshape(-1, 1) * grad[:K * B]).sum(0)
    return v, delta, G, theta


def test_layout_constants(hc):
    from gym_narde import _lib

    assert hc.hc_tdw_slab() == hc.hc_tdw_slab_macro() == _lib.TD_WINDOW_SLAB
    for n, k, h in ((1, 1, 1), (65, 7, 80), (63, 2, 17), (4096, 32, 128), (16384, 8, 80)):
        want = _lib.td_window_scratch_floats(n, k, h)
        assert hc.hc_tdw_scratch_floats(ctypes.c_int64(n), k, h) == want
        assert hc.hc_tdw_scratch_macro(ctypes.c_int64(n), k, h) == want


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_window_update_against_float64(hc, states, spec):
    net = make_net(*spec)
    p32, p64 = T.params_of(net, torch.float32), T.params_of(net, torch.float64)
    names = ("v", "delta", "G", "theta")
    worst = dict.fromkeys(names, 0.0)
    start = 0
    for K, B in SHAPES:
        for lam in (0.7, 1.0):
            board, off, player, feat = window(states, K, B, start)
            start += 97
            reward, term, trunc = flags(K, B, player)
            check_flags(K, B, player, reward, term, trunc)
            got = host_window(hc, net, board, off, player, reward, term, trunc, K, B, lam)
            r32 = reference(p32, feat, player, reward, term, trunc, K, B, lam, net.hidden_act, net.out_act)
            r64 = reference(p64, feat, player, reward, term, trunc, K, B, lam, net.hidden_act, net.out_act)
            moved = float((r64[3] - T.theta_row(p64)).abs().max())
            for name, g, a32, a64 in zip(names, got, r32, r64):
                b = T.Bound(f"{name} {spec[:3]} K={K} B={B} lam={lam}")
                b.add(g, a32.numpy(), a64.numpy())
                worst[name] = max(worst[name], b.check())
                if name == "theta":
                    e = max(b.e, float(np.spacing(np.float32(b.top))))
                    assert moved > 10 * T.TOL_FACTOR * e, (moved, e)  # an update lost would show
            # the ended plies cut the return: G = delta there
            ended = (term | trunc).astype(bool)
            assert np.array_equal(got[2][ended].view(np.int32), got[1][ended].view(np.int32))
            # a truncated ply's error is zero
            assert (got[1][(trunc == 1) & (term == 0)] == 0).all()
    print(f"worst ratios {spec[:3]}: " + ", ".join(f"{k} {v:.2f} E" for k, v in worst.items()))


@pytest.mark.parametrize("spec", NETS[:2], ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_lam_zero_gives_delta_bit_for_bit(hc, states, spec):
    net = make_net(*spec)
    for K, B in SHAPES:
        board, off, player, _ = window(states, K, B, 31)
        reward, term, trunc = flags(K, B, player)
        _, delta, G, _ = host_window(hc, net, board, off, player, reward, term, trunc, K, B, 0.0)
        assert not np.isnan(delta).any()
        assert np.array_equal(G.view(np.int32), delta.view(np.int32))
