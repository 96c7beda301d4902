"""The gradient forms of the two batch updates and the optimiser steps on a
given gradient (narde_rules.h "optimiser steps on a given gradient": what the
kernels of kernels_value_optim.h run) on the CPU, through a test-only host
build that runs the shared functions serially in the kernels' order
(tests/hostcheck/hostcheck_value_optim.cpp).

References: optim_ref (numpy, explicit formulas) in float64, itself checked
against torch.optim.AdamW / Adam (maximize=True) and clip_grad_norm_ in float64
within 1e-12 relative -- a reference against a reference --; the host steps
within 8 x E of it, E = max |optim_ref in float32 - optim_ref in float64| per
compared array, floored at one float32 ulp of its largest magnitude (td_ref's
rule, never a figure of the code under test), every hyperparameter the float32
value the call receives; the fold followed by the SGD element against the
existing host checks of the plain updates (hc_td_window, hc_value_fit), bit for
bit.
"""
import ctypes

import numpy as np
import pytest

import optim_ref as R
import td_ref as T

torch = pytest.importorskip("torch")

from test_td_window_cpu import ALPHA as W_ALPHA, GAMMA, NETS, P, flags, host_window, states, window  # noqa: E402,F401
from test_value_cpu import make_net  # noqa: E402
from test_value_fit_cpu import ALPHA as F_ALPHA, SENTINEL, _load, host_fit, samples, weights_of  # noqa: E402

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
STEPS, ZERO_STEP = 3, 1  # the second step's gradient is all zero
CHECKED = (1, 3)         # compared after these steps


@pytest.fixture(scope="module")
def ho():
    return _load("libhostcheck_value_optim.so")


@pytest.fixture(scope="module")
def hc_window():  # the plain windowed update's host check: the yardstick
    return _load("libhostcheck_td_window.so")


@pytest.fixture(scope="module")
def hc_fit():  # the plain fit's
    return _load("libhostcheck_value_fit.so")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def theta_of(arrays, H):
    w1t, b1, w2, b2, _ = arrays
    return np.concatenate([w1t[:, :H].reshape(-1), b1, w2, b2])


def net_args(arrays, H, pad):
    w1t, b1, w2, b2, w1 = arrays
    return (P(w1t), ctypes.c_int64(H + pad), P(b1), P(w2), P(b2), H, P(w1), ctypes.c_int64(198))


def check_mirror(arrays, H):
    w1t, _, _, _, w1 = arrays
    assert np.array_equal(bits(w1), bits(np.ascontiguousarray(w1t[:, :H].T)))
    assert (w1t[:, H:] == SENTINEL).all()  # the padding


def host_norm(ho, H, grad, max_norm):
    out = np.full(2, np.nan, np.float32)
    ho.hc_grad_norm(H, P(grad), ctypes.c_float(max_norm), P(out))
    return out


def test_layout_constants(ho):
    assert ho.hc_opt_state_bytes() == 24 and ho.hc_opt_block() == 256


# ------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_optim_ref_is_torchs_adamw_and_clip(wd):
    rows = 200 * 17 + 1
    grads = R.synthetic_grads(rows, STEPS, 3, 7, ZERO_STEP).astype(np.float64)
    theta0 = np.random.default_rng(1).normal(0, 0.3, rows)
    ref = R.Adam(theta0, weight_decay=wd, dtype=np.float64, **HYPER)
    kw = dict(lr=R.h(HYPER["lr"]), betas=tuple(R.h(b) for b in HYPER["betas"]), eps=R.h(HYPER["eps"]), maximize=True)
    runs = [(torch.optim.AdamW, dict(weight_decay=R.h(wd)))] + ([(torch.optim.Adam, {})] if wd == 0 else [])
    made = []
    for cls, extra in runs:
        p = torch.nn.Parameter(torch.from_numpy(theta0.copy()))
        made.append((p, cls([p], **kw, **extra)))
    for k in range(STEPS):
        norm, coef = R.clip(grads[k], 1.0, np.float64)
        for p, opt in made:
            p.grad = torch.from_numpy(grads[k].copy())
            total = torch.nn.utils.clip_grad_norm_([p], R.h(1.0))
            assert abs(float(total) - norm) <= 1e-12 * max(norm, 1e-300)
            want = grads[k] * coef
            assert np.abs(p.grad.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
            opt.step()
        ref.step(grads[k], scale=coef)
        for p, opt in made:
            assert np.abs(p.detach().numpy() - ref.theta).max() <= 1e-12 * np.abs(ref.theta).max(), (type(opt), k)
            st = opt.state[p]
            # (maximize: torch keeps the moment of the negated gradient)
            assert np.abs(-st["exp_avg"].numpy() - ref.m).max() <= 1e-12 * max(np.abs(ref.m).max(), 1e-300)
            assert np.abs(st["exp_avg_sq"].numpy() - ref.s).max() <= 1e-12 * max(np.abs(ref.s).max(), 1e-300)
    assert np.abs(ref.theta - theta0).max() > 1e-4  # it did move


# ------------------------------------------------------------------ the host steps against the reference
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip1"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("H", [1, 2, 17, 80, 128])
def test_host_adam_against_float64(ho, H, wd, clip):
    net = make_net(H, "sigmoid", "tanh", seed=H)
    pad = 4
    arrays = weights_of(net, pad)
    rows = 200 * H + 1
    grads = R.synthetic_grads(rows, STEPS, 100 + H, 7, ZERO_STEP)
    theta0 = theta_of(arrays, H)
    refs = [R.Adam(theta0, weight_decay=wd, dtype=dt, **HYPER) for dt in (np.float32, np.float64)]
    m, s = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
    state = np.zeros(3, np.int64)
    worst = 0.0
    for k in range(STEPS):
        scale = None
        if clip is not None:
            out = host_norm(ho, H, grads[k], clip)
            c32, c64 = R.clip(grads[k], clip, np.float32), R.clip(grads[k], clip, np.float64)
            scale = out[1:].copy()
        ho.hc_adam_step(*net_args(arrays, H, pad), P(grads[k]), P(scale) if scale is not None else None, P(m), P(s),
                        P(state), ctypes.c_float(HYPER["lr"]), ctypes.c_float(HYPER["betas"][0]),
                        ctypes.c_float(HYPER["betas"][1]), ctypes.c_float(HYPER["eps"]), ctypes.c_float(wd))
        for ref, c in zip(refs, (c32, c64) if clip is not None else (None, None)):
            ref.step(grads[k], scale=None if c is None else c[1])
        if k + 1 in CHECKED:
            what = f"H={H} wd={wd} clip={clip} step {k + 1}"
            got = dict(theta=theta_of(arrays, H), m=m, s=s)
            if clip is not None:
                got.update(norm=out[:1], scale=out[1:])
            for key, g in got.items():
                a32, a64 = ((c32, c64)[i][("norm", "scale").index(key)] if key in ("norm", "scale")
                            else getattr(refs[i], key) for i in (0, 1))
                b = T.Bound(f"{key} {what}")
                b.add(g, a32, a64)
                worst = max(worst, b.check())
            check_mirror(arrays, H)
    assert state[0] == STEPS
    pows = state[1:].view(np.float64)
    assert abs(pows[0] - R.h(0.9) ** 3) < 1e-15 and abs(pows[1] - R.h(0.999) ** 3) < 1e-15
    assert np.abs(theta_of(arrays, H) - theta0).max() > 100 * np.spacing(np.float32(np.abs(theta0).max()))  # it moved
    print(f"worst ratio H={H} wd={wd} clip={clip}: {worst:.2f} E")


@pytest.mark.parametrize("H", [1, 17, 128])
def test_host_norm_and_sgd_against_float64(ho, H):
    net = make_net(H, "tanh", "none", seed=H + 1)
    rows = 200 * H + 1
    grads = R.synthetic_grads(rows, STEPS, 200 + H, 7, ZERO_STEP)
    alpha = 1e-3
    for k in (0, ZERO_STEP):
        g = grads[k]
        n64 = R.clip(g, 1.0, np.float64)[0]
        for max_norm in (0.0, 1.0, float(n64) * 0.5, float(n64) * 4 + 1.0):
            out = host_norm(ho, H, g, max_norm)
            c32, c64 = R.clip(g, max_norm, np.float32), R.clip(g, max_norm, np.float64)
            for i, key in enumerate(("norm", "scale")):
                b = T.Bound(f"{key} H={H} step {k} max_norm={max_norm:.3g}")
                b.add(out[i:i + 1], c32[i], c64[i])
                b.check()
            if max_norm > n64:
                assert out[1] == 1.0  # exactly: an unclipped step
            elif n64 > 0:
                assert out[1] < 1.0
            arrays, plain = weights_of(net, 4), weights_of(net, 4)
            theta0 = theta_of(arrays, H)
            ho.hc_sgd_step(*net_args(arrays, H, 4), P(g), P(out[1:].copy()), ctypes.c_float(alpha))
            ho.hc_sgd_step(*net_args(plain, H, 4), P(g), None, ctypes.c_float(alpha))
            r32, r64 = (R.sgd(theta0, g, alpha, dt, scale=c[1]) for dt, c in ((np.float32, c32), (np.float64, c64)))
            b = T.Bound(f"theta H={H} step {k} max_norm={max_norm:.3g}")
            b.add(theta_of(arrays, H), r32, r64)
            b.check()
            check_mirror(arrays, H)
            if out[1] == 1.0:  # an unclipped step's bits
                assert np.array_equal(bits(theta_of(arrays, H)), bits(theta_of(plain, H)))
            if k == ZERO_STEP or max_norm == 0.0:  # nothing to add
                assert np.array_equal(bits(theta_of(arrays, H)), bits(theta0))


# ------------------------------------------------------------------ the fold and the SGD element: the plain updates' bits
@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_window_grad_then_sgd_is_the_plain_windows_bits(ho, hc_window, states, spec):
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    net = make_net(*spec)
    H = net.hidden
    for (K, B), lam in (((1, 1), 0.7), ((2, 65), 0.7), ((7, 65), 1.0)):
        board, off, player, _ = window(states, K, B, 41)
        reward, term, trunc = flags(K, B, player)
        v0, d0, G0, theta_plain = host_window(hc_window, net, board, off, player, reward, term, trunc, K, B, lam)
        arrays = weights_of(net)
        theta0 = theta_of(arrays, H)
        w1t, b1, w2, b2, _ = arrays
        v = np.full((K + 1) * B, np.nan, np.float32)
        delta, G = np.full(K * B, np.nan, np.float32), np.full(K * B, np.nan, np.float32)
        grad = np.full(200 * H + 1, np.nan, np.float32)
        c = np.ascontiguousarray
        ho.hc_td_window_grad(K, ctypes.c_int64(B), P(board), P(off), P(player), P(c(reward)), P(c(term)), P(c(trunc)),
                             P(w1t), ctypes.c_int64(H), P(b1), P(w2), P(b2), H, HIDDEN_ACTS[net.hidden_act],
                             OUT_ACTS[net.out_act], ctypes.c_float(lam), ctypes.c_float(GAMMA), P(v), P(delta), P(G),
                             P(grad))
        assert np.array_equal(bits(theta_of(arrays, H)), bits(theta0))  # the gradient call moves no weight
        assert not np.isnan(grad).any() and np.abs(grad).max() > 0
        for got, want in ((v, v0), (delta, d0), (G, G0)):
            assert np.array_equal(bits(got), bits(want.reshape(-1)))
        ho.hc_sgd_step(*net_args(arrays, H, 0), P(grad), None, ctypes.c_float(W_ALPHA))
        assert np.array_equal(bits(theta_of(arrays, H)), bits(theta_plain)), (spec, K, B)
        assert not np.array_equal(bits(theta_plain), bits(theta0))
        check_mirror(arrays, H)


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_fit_grad_then_sgd_is_the_plain_fits_bits(ho, hc_fit, states, spec):
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    net = make_net(*spec)
    H = net.hidden
    rng = np.random.default_rng(spec[3])
    for n in (1, 127, 129, 300):
        board, off, player, _ = samples(states, n, 53)
        target = (rng.random(n) * 4 - 2).astype(np.float32)
        mixed = rng.random(n).astype(np.float32) * 2
        zero = (np.arange(n) % 3 == 0) if n > 1 else np.array([False])
        mixed[zero] = 0.0
        t_nan = target.copy()
        t_nan[zero] = np.nan  # never read
        for tg, wt in ((target, None), (t_nan, mixed)):
            plain = host_fit(hc_fit, net, board, off, player, tg, wt)
            arrays = weights_of(net)
            theta0 = theta_of(arrays, H)
            w1t, b1, w2, b2, _ = arrays
            v, loss = np.full(n, np.nan, np.float32), np.full(2, np.nan, np.float64)
            grad = np.full(200 * H + 1, np.nan, np.float32)
            c = np.ascontiguousarray
            ho.hc_value_fit_grad(ctypes.c_int64(n), P(c(board)), P(c(off)), P(c(player)), P(tg),
                                 P(wt) if wt is not None else None, P(w1t), ctypes.c_int64(H), P(b1), P(w2), P(b2), H,
                                 HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act], P(v), P(loss), P(grad))
            assert np.array_equal(bits(theta_of(arrays, H)), bits(theta0))  # the gradient call moves no weight
            assert not np.isnan(grad).any()
            assert np.array_equal(bits(v), bits(plain["v"])) and np.array_equal(loss, plain["loss"])
            ho.hc_sgd_step(*net_args(arrays, H, 0), P(grad), None, ctypes.c_float(F_ALPHA))
            assert np.array_equal(bits(theta_of(arrays, H)), bits(plain["theta"])), (spec, n)
            check_mirror(arrays, H)
