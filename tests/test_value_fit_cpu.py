"""The supervised fit and the playout targets (narde_rules.h "the value MLP's
supervised fit": what narde_value_fit's and narde_playout_targets' kernels run)
on the CPU, through a test-only host build that runs the shared functions
serially in the kernels' summation order
(tests/hostcheck/hostcheck_value_fit.cpp), on the golden states with every
third mover flipped.

References: narde.h's semantics in torch float64 -- td_ref.value_and_grad for v
and the gradient rows, theta + alpha sum w (t - v) grad v -- within 8 x E, E =
max |the same formulas in float32 - float64| per compared array (td_ref's
rule); the loss as a numpy float64 restatement in the stated two-level order,
exactly; the existing windowed update (hc_td_window) on an all-terminated
window, bit for bit; the targets as a float64 numpy restatement and the
existing pick's score (hc_playout_pick), exactly.
"""
import ctypes
import os

import numpy as np
import pytest

import td_ref as T
from conftest import ROOT

torch = pytest.importorskip("torch")

from test_td_window_cpu import NETS, P, states  # noqa: E402,F401  (states: a fixture)
from test_value_cpu import make_net  # noqa: E402

SHAPES = (1, 4, 127, 128, 129, 300)
ALPHA = 0.05
SLAB = 128
SENTINEL = np.float32(-12345.5)
TAIL = 16  # sentinel floats behind the scratch's stated size


def _load(name):
    path = os.path.join(ROOT, "tests", "hostcheck", "build", name)
    if not os.path.exists(path):
        pytest.fail(f"tests/hostcheck/build/{name} is missing: run __graft_entry__.build()")
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def hc():
    lib = _load("libhostcheck_value_fit.so")
    lib.hc_fit_scratch_floats.restype = ctypes.c_int64
    lib.hc_fit_scratch_macro.restype = ctypes.c_int64
    return lib


def samples(states, n, start):
    board, off, player, feat = states
    sl = slice(start, start + n)
    assert sl.stop <= len(player)
    return board[sl], off[sl], player[sl], feat[sl]


def weights_of(net, pad=0):
    """(w1t [198][H + pad], b1, w2, b2, w1 [H][198]) float32 copies; the padding holds a sentinel"""
    H = net.hidden
    w1 = np.ascontiguousarray(net.l1.weight.detach().numpy(), dtype=np.float32).copy()
    w1t = np.full((198, H + pad), SENTINEL, np.float32)
    w1t[:, :H] = w1.T
    b1 = net.l1.bias.detach().numpy().astype(np.float32).copy()
    w2 = net.l2.weight.detach().numpy().reshape(-1).astype(np.float32).copy()
    b2 = net.l2.bias.detach().numpy().astype(np.float32).copy()
    return w1t, b1, w2, b2, w1


def host_fit(hc, net, board, off, player, target, weight=None, alpha=ALPHA, pad=0, start=None):
    """One hc_value_fit on a copy of the net's weights (or on `start`, an
    earlier result's weights).  Returns a dict: v, loss, theta (a trace row's
    layout), the weight arrays, the scratch's tail."""
    from gym_narde import _lib
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    H, n = net.hidden, len(player)
    w1t, b1, w2, b2, w1 = (a.copy() for a in start) if start is not None else weights_of(net, pad)
    need = _lib.value_fit_scratch_floats(n, H)
    scratch = np.full(need + TAIL, SENTINEL, np.float32)
    assert scratch.ctypes.data % 8 == 0
    v = np.full(n, np.nan, np.float32)
    loss = np.full(2, np.nan, np.float64)
    c = np.ascontiguousarray
    hc.hc_value_fit(ctypes.c_int64(n), P(c(board)), P(c(off)), P(c(player)), P(c(target, dtype=np.float32)),
                    P(c(weight, dtype=np.float32)) if weight is not None else None, P(w1t), ctypes.c_int64(H + pad),
                    P(b1), P(w2), P(b2), H, HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act], P(w1),
                    ctypes.c_int64(198), ctypes.c_float(alpha), P(scratch), P(v), P(loss))
    theta = np.concatenate([w1t[:, :H].reshape(-1), b1, w2, b2])
    return dict(v=v, loss=loss, theta=theta, arrays=(w1t, b1, w2, b2, w1), tail=scratch[need:])


def loss_restated(v, target, weight):
    """{sum w e^2, sum w}: e = target - v in float32; per slab of 128, in
    sample order, in float64, (w e) e; a zero weight adds nothing; then the
    slabs in slab order."""
    n = len(v)
    tot = [np.float64(0.0), np.float64(0.0)]
    for s0 in range(0, n, SLAB):
        se, sw = np.float64(0.0), np.float64(0.0)
        for i in range(s0, min(s0 + SLAB, n)):
            w = np.float32(1.0) if weight is None else np.float32(weight[i])
            if w == 0:
                continue
            e = np.float32(target[i]) - np.float32(v[i])
            se = se + (np.float64(w) * np.float64(e)) * np.float64(e)
            sw = sw + np.float64(w)
        tot[0], tot[1] = tot[0] + se, tot[1] + sw
    return np.array(tot, np.float64)


def reference(params, feat, target, weight, alpha, hidden_act, out_act):
    """narde.h's semantics in params' dtype: (v, theta)."""
    dt = params[0].dtype
    v, grad = T.value_and_grad(params, torch.from_numpy(feat).to(dt), hidden_act, out_act)
    t = torch.from_numpy(np.nan_to_num(np.asarray(target, np.float32), nan=0.0)).to(dt)
    w = torch.ones_like(t) if weight is None else torch.from_numpy(np.asarray(weight, np.float32)).to(dt)
    G = torch.where(w == 0, torch.zeros_like(t), w * (t - v))
    return v, T.theta_row(params) + torch.tensor(alpha, dtype=dt) * (G.reshape(-1, 1) * grad).sum(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_layout_constants(hc):
    from gym_narde import _lib

    assert hc.hc_fit_slab() == hc.hc_fit_slab_macro() == _lib.VALUE_FIT_SLAB == SLAB
    for n, h in ((1, 1), (300, 80), (127, 17), (128, 128), (129, 128), (2 ** 31 - 1, 128)):
        want = _lib.value_fit_scratch_floats(n, h)
        assert hc.hc_fit_scratch_floats(ctypes.c_int64(n), h) == want
        assert hc.hc_fit_scratch_macro(ctypes.c_int64(n), h) == want
    assert _lib.value_fit_scratch_floats(1, 1) == 208 and _lib.value_fit_scratch_floats(300, 80) == 3 * 16008


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_fit_against_float64(hc, states, spec):
    net = make_net(*spec)
    p32, p64 = T.params_of(net, torch.float32), T.params_of(net, torch.float64)
    worst = {"v": 0.0, "theta": 0.0}
    rng = np.random.default_rng(spec[3])
    start = 0
    for n in SHAPES:
        board, off, player, feat = samples(states, n, start)
        start += 97
        target = (rng.random(n) * 4 - 2).astype(np.float32)
        mixed = rng.random(n).astype(np.float32) * 2
        zero = (np.arange(n) % 3 == 0) if n > 1 else np.array([False])
        mixed[zero] = 0.0
        t_nan = target.copy()
        t_nan[zero] = np.nan  # never read
        base = host_fit(hc, net, board, off, player, target)
        for name, tg, wt in (("NULL", target, None), ("ones", target, np.ones(n, np.float32)), ("mixed", t_nan, mixed)):
            got = host_fit(hc, net, board, off, player, tg, wt, pad=4)
            r32 = reference(p32, feat, tg, wt, ALPHA, net.hidden_act, net.out_act)
            r64 = reference(p64, feat, tg, wt, ALPHA, net.hidden_act, net.out_act)
            moved = float((r64[1] - T.theta_row(p64)).abs().max())
            for key, g, a32, a64 in zip(("v", "theta"), (got["v"], got["theta"]), r32, r64):
                b = T.Bound(f"{key} {spec[:3]} n={n} weights={name}")
                b.add(g, a32.numpy(), a64.numpy())
                worst[key] = max(worst[key], b.check())
                if key == "theta":
                    e = max(b.e, float(np.spacing(np.float32(b.top))))
                    assert moved > 10 * T.TOL_FACTOR * e, (moved, e)  # an update lost would show
            assert np.array_equal(got["loss"], loss_restated(got["v"], tg, wt)), (n, name)
            assert not np.isnan(got["loss"]).any() and got["loss"][1] > 0
            assert np.array_equal(bits(got["v"]), bits(base["v"]))  # v does not depend on the weights
            w1t, _, _, _, w1 = got["arrays"]
            assert np.array_equal(bits(w1), bits(np.ascontiguousarray(w1t[:, :net.hidden].T)))  # the mirror
            assert (w1t[:, net.hidden:] == SENTINEL).all()  # ld_w1t = H + 4: the padding
            assert (got["tail"] == SENTINEL).all()
            if name == "ones":
                assert np.array_equal(bits(got["theta"]), bits(base["theta"]))
                assert np.array_equal(got["loss"], base["loss"])
    print(f"worst ratios {spec[:3]}: " + ", ".join(f"{k} {v:.2f} E" for k, v in worst.items()))


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_what_leaves_the_weights_as_they_were(hc, states, spec):
    net = make_net(*spec)
    theta0 = np.concatenate([a.reshape(-1) for a in weights_of(net)[:4]])
    rng = np.random.default_rng(7)
    for n in (4, 129, 300):
        board, off, player, _ = samples(states, n, 11)
        target = (rng.random(n) * 4 - 2).astype(np.float32)
        # every weight zero, the targets NaN: nothing is read, nothing moves, the loss is {0, 0}
        got = host_fit(hc, net, board, off, player, np.full(n, np.nan, np.float32), np.zeros(n, np.float32))
        assert np.array_equal(bits(got["theta"]), bits(theta0)) and np.array_equal(got["loss"], [0.0, 0.0])
        assert np.array_equal(bits(got["arrays"][4]), bits(weights_of(net)[4]))
        # alpha = 0: a validation loss
        val = host_fit(hc, net, board, off, player, target, alpha=0.0)
        assert np.array_equal(bits(val["theta"]), bits(theta0))
        assert np.array_equal(val["loss"], loss_restated(val["v"], target, None)) and val["loss"][0] > 0
        assert val["loss"][1] == n
        # target = the call's own v: every error is zero
        again = host_fit(hc, net, board, off, player, val["v"], alpha=ALPHA)
        assert np.array_equal(bits(again["theta"]), bits(theta0)) and again["loss"][0] == 0.0 and again["loss"][1] == n
        assert np.array_equal(bits(again["v"]), bits(val["v"]))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_all_terminated_window_gives_the_window_updates_bits(hc, states, spec, K):
    """The yardstick is the existing windowed update (hc_td_window), not the
    code under test: every ply terminated, gamma = 1, so G_k = outcome - v_k."""
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    hw = _load("libhostcheck_td_window.so")
    B = 65
    net = make_net(*spec)
    board, off, player, _ = samples(states, (K + 1) * B, 29)
    n = K * B
    black = player[:n] == -1
    reward = (1 + (np.arange(n) // 2) % 2).astype(np.int32)
    combos = {(int(r), bool(b)) for r, b in zip(reward, black)}
    assert combos == {(1, False), (1, True), (2, False), (2, True)}
    term, trunc = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    w1t, b1, w2, b2, _ = weights_of(net)
    H = net.hidden
    v, delta, G = (np.full(m, np.nan, np.float32) for m in ((K + 1) * B, n, n))
    hw.hc_td_window(K, ctypes.c_int64(B), P(board), P(off), P(player), P(reward), P(term), P(trunc), P(w1t),
                    ctypes.c_int64(H), P(b1), P(w2), P(b2), H, HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act],
                    ctypes.c_float(ALPHA), ctypes.c_float(0.7), ctypes.c_float(1.0), P(v), P(delta), P(G))
    window_theta = np.concatenate([w1t.reshape(-1), b1, w2, b2])
    target = np.where(black, -reward, reward).astype(np.float32)
    got = host_fit(hc, net, board[:n], off[:n], player[:n], target)
    assert np.array_equal(bits(got["v"]), bits(v[:n]))
    assert np.array_equal(bits(got["theta"]), bits(window_theta))
    assert not np.array_equal(bits(got["theta"]), bits(np.concatenate([a.reshape(-1) for a in weights_of(net)[:4]])))


# ------------------------------------------------------------------ the targets
def numpy_targets(sums, leaf, trials, roots):
    n = sums.shape[0]
    target, weight = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        if roots is not None and ((int(roots[i, 6]) & 15) == 15 or ((int(roots[i, 6]) >> 4) & 15) == 15):
            continue
        fin, pts = int(sums[i, 0]), int(sums[i, 1])
        if leaf is None:
            if fin > 0:
                target[i], weight[i] = np.float32(np.float64(pts) / np.float64(fin)), 1.0
        else:
            S = np.float64(0.0)
            for j in range(trials):
                if not np.isnan(leaf[i, j]):
                    S = S + np.float64(leaf[i, j])
            target[i], weight[i] = np.float32((np.float64(pts) + S) / np.float64(trials)), 1.0
    return target, weight


def host_targets(hc, sums, leaf, trials, roots):
    n = sums.shape[0]
    target, weight = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    hc.hc_playout_targets(ctypes.c_int64(n), trials, P(sums), P(leaf) if leaf is not None else None,
                          P(roots) if roots is not None else None, P(target), P(weight))
    return target, weight


@pytest.fixture(scope="module")
def playouts():
    """hc_value_playout (REF2) on every 9th start state and the four endgames,
    6 plies, 4 trials; behind them the none record and a finished game's record
    with made-up sums."""
    from test_playout_pick_cpu import NONE6
    from test_value_playout_cpu import PLIES, host_playout, some
    from test_value_rollout_cpu import BLACK, start_states

    hp = _load("libhostcheck_playout_pick.so")
    trials = 4
    st = some(tuple(a.copy() for a in start_states()[:4]), 9)
    res = host_playout(hp, "ref2", st, 0, trials, PLIES, make_net(*NETS[0]), make_net(*BLACK[80]))
    none = np.zeros((2, 8), np.uint32)
    none[0, 6] = NONE6
    none[1, 6] = 15 | (3 << 4)  # white has borne off all 15
    none[1, 2] = 0x00000444
    roots = np.ascontiguousarray(np.concatenate([res["records"], none]))
    sums = np.ascontiguousarray(np.concatenate([res["sums"], np.array([[4, 4, 4, 8], [2, -2, 2, 9]], np.int32)]))
    leaf = np.ascontiguousarray(np.concatenate([res["leaf"], np.array([[np.nan] * 4, [0.5, np.nan, np.nan, 0.25]],
                                                                      np.float32)]))
    return hp, trials, roots, sums, leaf


@pytest.mark.parametrize("with_leaf", [False, True], ids=["finished-mean", "truncated-mean"])
@pytest.mark.parametrize("with_roots", [False, True], ids=["no-roots", "roots"])
def test_targets_are_the_float64_restatement_and_the_picks_score(hc, playouts, with_leaf, with_roots):
    from test_playout_pick_cpu import host_playout_pick

    hp, trials, roots, sums, leaf = playouts
    n = sums.shape[0]
    fin = sums[:, 0]
    # from the sums: roots no trial finished, roots some or all finished
    assert (fin[:-2] == 0).any() and ((fin[:-2] > 0) & (fin[:-2] < trials)).any() | (fin[:-2] == trials).any()
    assert (fin[-6:-2] == trials).all()  # the endgames
    lf, rt = (leaf if with_leaf else None), (roots if with_roots else None)
    target, weight = host_targets(hc, sums, lf, trials, rt)
    want_t, want_w = numpy_targets(sums, lf, trials, rt)
    assert np.array_equal(bits(target), bits(want_t)) and np.array_equal(bits(weight), bits(want_w))
    assert set(np.unique(weight)) <= {0.0, 1.0}
    if with_roots:
        assert weight[-1] == 0 and weight[-2] == 0 and target[-1] == 0 and target[-2] == 0
    else:
        assert weight[-1] == 1 and weight[-2] == 1
    if not with_leaf or with_roots:
        assert (weight == 0).any()
    if not with_leaf:
        assert (weight[fin == 0] == 0).all() and (target[fin == 0] == 0).all()
    # the pick's score of a non-terminal slot (k = 1, slot i = row i), bit for bit
    sel = np.arange(n, dtype=np.int32).reshape(n, 1)
    _, _, score = host_playout_pick(hp, "ref2", sel, n, np.zeros(n, np.float32), np.zeros(n, np.int8),
                                    np.zeros((n, 2), np.int16), trials, sums, lf, np.zeros(n, np.uint8))
    live = weight == 1
    assert live.sum() >= 4
    assert np.array_equal(bits(target[live]), bits(score.reshape(-1)[live]))
