"""The gradient forms of the two batch updates and the optimiser steps on the
GPU: narde_value_td_window_grad, narde_value_fit_grad,
narde_value_grad_norm, narde_value_sgd_step, narde_value_adam_step
(kernels_value_optim.h), gym_narde.td.ValueSGD / ValueAdam and the learners'
optimizer= and grad_hook=.

Yardsticks: the plain calls (narde_value_td_window, narde_value_fit) bit for
bit; td_ref.value_and_grad rows in float64 for the gradient's values; optim_ref
in float64 for the steps.  Tolerance: 8 x E, E = max |the same formulas in
float32 - float64| per compared array, floored at one float32 ulp of its
largest magnitude -- td_ref's rule, never a figure of the code under test;
every hyperparameter enters the restatements as the float32 value the call
receives.
"""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import optim_ref as R
import td_ref as T
from conftest import ROOT
from test_value_cpu import make_net

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import np_  # noqa: E402
from test_gpu_td_window import DEV, SENT, RawNet, middle_game, window_inputs  # noqa: E402
from test_gpu_value_fit import ACTS, fit_call, recorded  # noqa: E402,F401  (recorded: a fixture)

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
STEPS, ZERO_STEP = 3, 1  # the second step's gradient is all zero
GAMMA, LAM, ALPHA = 0.9, 0.7, 0.01


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def lib():
    from gym_narde import _lib

    return _lib


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def f32(a, dev=DEV):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float32)).to(dev)


def guarded(n, dtype=torch.float32):
    """n elements with four sentinels behind them."""
    return torch.full((n + 4,), SENT, dtype=dtype, device=DEV)


# ------------------------------------------------------------------ the C calls
def window_call(env, mlp, plies, bufs, H, alpha=None):
    """narde_value_td_window (alpha given) or narde_value_td_window_grad (None):
    (v, delta, G, grad or None) on the host, sentinels checked."""
    L = lib()
    B, P = env.num_envs, 200 * H + 1
    n = L.td_window_scratch_floats(B, plies, H)
    scratch, delta, grad = guarded(n), guarded(plies * B), guarded(P)
    head = (ctypes.byref(mlp), plies, L.ptr(bufs["records"]), L.ptr(bufs["reward"]), L.ptr(bufs["terminated"]),
            L.ptr(bufs["truncated"]))
    if alpha is None:
        env.handle.call("narde_value_td_window_grad", *head, LAM, GAMMA, L.ptr(scratch), n, L.ptr(delta), L.ptr(grad),
                        env._s())
    else:
        env.handle.call("narde_value_td_window", *head, alpha, LAM, GAMMA, L.ptr(scratch), n, L.ptr(delta), env._s())
    torch.cuda.synchronize()
    assert (scratch[n:] == SENT).all() and (delta[plies * B:] == SENT).all() and (grad[P:] == SENT).all()
    all_, stored = (plies + 1) * B, plies * B
    g0 = (all_ + 3) // 4 * 4
    return np_(scratch[:all_]), np_(delta[:stored]), np_(scratch[g0:g0 + stored]), (np_(grad[:P]) if alpha is None else None)


def fit_grad_call(env, mlp, records, target, weight, H):
    """narde_value_fit_grad: (v, loss, grad) on the host, sentinels checked."""
    L = lib()
    n, P = int(records.shape[0]), 200 * H + 1
    need = L.value_fit_scratch_floats(n, H)
    scratch, v, grad = guarded(need), guarded(n), guarded(P)
    loss = torch.full((2,), SENT, dtype=torch.float64, device=DEV)
    tg, wt = f32(target), f32(weight)
    L.check(env.handle.lib.narde_value_fit_grad(env.device.index, ctypes.byref(mlp), n, L.ptr(records), L.ptr(tg),
                                                L.ptr(wt), L.ptr(scratch), need, L.ptr(v), L.ptr(loss), L.ptr(grad),
                                                env._s()), "narde_value_fit_grad")
    torch.cuda.synchronize()
    assert (scratch[need:] == SENT).all() and (v[n:] == SENT).all() and (grad[P:] == SENT).all()
    return np_(v[:n]), np_(loss), np_(grad[:P])


def norm_call(H, grad, max_norm):
    """narde_value_grad_norm: the device tensor out (2,), a sentinel behind it checked."""
    L = lib()
    out = guarded(2)
    L.check(L.load().narde_value_grad_norm(0, H, L.ptr(grad), max_norm, L.ptr(out), stream()), "narde_value_grad_norm")
    torch.cuda.synchronize()
    assert (out[2:] == SENT).all()
    return out[:2]


def sgd_call(mlp, grad, scale, alpha):
    L = lib()
    L.check(L.load().narde_value_sgd_step(0, ctypes.byref(mlp), L.ptr(grad), L.ptr(scale), alpha, stream()),
            "narde_value_sgd_step")
    torch.cuda.synchronize()


def adam_call(mlp, grad, scale, m, s, state, wd):
    L = lib()
    L.check(L.load().narde_value_adam_step(0, ctypes.byref(mlp), L.ptr(grad), L.ptr(scale), L.ptr(m), L.ptr(s),
                                           L.ptr(state), HYPER["lr"], HYPER["betas"][0], HYPER["betas"][1],
                                           HYPER["eps"], wd, stream()), "narde_value_adam_step")
    torch.cuda.synchronize()


def check(what, got, x32, x64):
    b = T.Bound(what)
    b.add(got, np.asarray(x32), np.asarray(x64))
    return b.check()


# ------------------------------------------------------------------ 1, 3: the window's gradient
def window_grad_reference(p, feat, player, reward, term, trunc, v_call, K, B, acts):
    """sum_i G_i grad v(s_i) in p's dtype, G from the call's own v."""
    dt = p[0].dtype
    _, rows = T.value_and_grad(p, torch.from_numpy(feat[:K * B]).to(dt), *acts)
    v = torch.from_numpy(v_call).to(dt).reshape(K + 1, B)
    tm, tr = torch.from_numpy(term), torch.from_numpy(trunc)
    gamma = torch.tensor(R.h(GAMMA), dtype=dt)
    delta = T.td_targets(v[:K], v[1:], torch.from_numpy(reward), torch.from_numpy((player[:K * B] == -1).reshape(K, B)),
                         tm, tr, gamma)
    c = torch.where((tm | tr).bool(), torch.zeros((), dtype=dt), gamma * torch.tensor(R.h(LAM), dtype=dt))
    G, nxt = torch.zeros_like(delta), torch.zeros(B, dtype=dt)
    for k in range(K - 1, -1, -1):
        nxt = delta[k] + c[k] * nxt
        G[k] = nxt
    return (G.reshape(-1, 1) * rows).sum(0).numpy()


WINDOW_CASES = [(H, ("ref2", "full4")[(i + j) % 2], 4 * ((i + j + 1) % 2), ACTS[(3 * i + j) % 9])
                for i, H in enumerate((1, 17, 80, 128)) for j in range(2)]


@pytest.mark.parametrize("H,rules,pad,acts", WINDOW_CASES, ids=lambda x: "-".join(x) if isinstance(x, tuple) else str(x))
def test_window_grad_then_sgd_is_the_plain_windows_bits(H, rules, pad, acts):
    B, K = 65, 3
    env = middle_game(rules, B)
    cpu = make_net(H, *acts, seed=H + 3)
    net = copy.deepcopy(cpu).to(env.device)
    make = env.turn_value_rollout_buffers if env.full else env.value_rollout_buffers
    bufs = make(K, records=True)
    (env.turn_value_rollout if env.full else env.value_rollout)(K, net, epsilon=0.2, tag=0, seed=4, bufs=bufs)
    plain, split = RawNet(cpu, env.device, pad), RawNet(cpu, env.device, pad)
    theta0 = plain.theta()
    p32, p64 = split.params(torch.float32), split.params(torch.float64)
    v0, d0, G0, _ = window_call(env, plain.mlp, K, bufs, H, alpha=ALPHA)
    v1, d1, G1, grad = window_call(env, split.mlp, K, bufs, H)
    # after the gradient call alone no weight bit has moved
    assert np.array_equal(bits(split.theta()), bits(theta0))
    fresh = RawNet(cpu, env.device, pad)
    assert same_bits(split.w1t, fresh.w1t) and same_bits(split.w1, fresh.w1)
    for a, b in ((v0, v1), (d0, d1), (G0, G1)):
        assert np.array_equal(bits(a), bits(b))
    # its values
    feat, player, reward, term, trunc = window_inputs(bufs, env, K)
    r32, r64 = (window_grad_reference(p, feat, player, reward, term, trunc, v1, K, B, acts) for p in (p32, p64))
    what = f"H={H} {acts[0]}/{acts[1]} {rules} pad={pad}"
    ratio = check(f"window grad {what}", grad, r32, r64)
    assert np.abs(r64).max() > 0
    # the step: the plain call's weight and mirror bits
    sgd_call(split.mlp, f32(grad), None, ALPHA)
    assert np.array_equal(bits(split.theta()), bits(plain.theta())) and not np.array_equal(bits(plain.theta()), bits(theta0))
    assert same_bits(split.w1t, plain.w1t) and same_bits(split.w1, plain.w1)
    assert same_bits(split.b1, plain.b1) and same_bits(split.w2, plain.w2) and same_bits(split.b2, plain.b2)
    plain.checks()
    split.checks()
    print(f"window grad {what}: {ratio:.2f} E")
    env.close()


# ------------------------------------------------------------------ 2, 3: the fit's gradient
def fit_grad_reference(p, feat, target, weight, v_call, acts):
    dt = p[0].dtype
    _, rows = T.value_and_grad(p, torch.from_numpy(feat).to(dt), *acts)
    t = torch.from_numpy(np.nan_to_num(np.asarray(target, np.float32), nan=0.0)).to(dt)
    w = torch.ones_like(t) if weight is None else torch.from_numpy(np.asarray(weight, np.float32)).to(dt)
    G = torch.where(w == 0, torch.zeros_like(t), w * (t - torch.from_numpy(v_call).to(dt)))
    return (G.reshape(-1, 1) * rows).sum(0).numpy()


FIT_CASES = [(n, H, ACTS[(i + 2 * j) % 9], ("ref2", "full4")[(i + j) % 2], 4 * ((i + j) % 2))
             for i, n in enumerate((1, 127, 129, 300)) for j, H in enumerate((1, 17, 80, 128))]


@pytest.mark.parametrize("n,H,acts,rules,pad", FIT_CASES, ids=lambda x: "-".join(x) if isinstance(x, tuple) else str(x))
def test_fit_grad_then_sgd_is_the_plain_fits_bits(recorded, n, H, acts, rules, pad):  # noqa: F811
    env, records, feat, target = recorded[rules]
    start = (7 * n + H) % (len(target) - n + 1)
    rec, ft, tg = records[start:start + n].contiguous(), feat[start:start + n], target[start:start + n]
    cpu = make_net(H, *acts, seed=H + n)
    mixed = np.random.default_rng(n).random(n).astype(np.float32) * 2
    zero = (np.arange(n) % 3 == 0) if n > 1 else np.array([False])
    mixed[zero] = 0.0
    t_nan = tg.copy()
    t_nan[zero] = np.nan  # never read
    what = f"n={n} H={H} {acts[0]}/{acts[1]} {rules} pad={pad}"
    worst = 0.0
    for name, t_in, w_in in (("NULL", tg, None), ("ones", tg, np.ones(n, np.float32)), ("mixed", t_nan, mixed)):
        plain, split = RawNet(cpu, env.device, pad), RawNet(cpu, env.device, pad)
        theta0 = plain.theta()
        p32, p64 = split.params(torch.float32), split.params(torch.float64)
        v0, loss0 = fit_call(env, plain.mlp, rec, t_in, w_in, ALPHA, H)
        v1, loss1, grad = fit_grad_call(env, split.mlp, rec, t_in, w_in, H)
        assert np.array_equal(bits(split.theta()), bits(theta0))  # the gradient call alone moves no weight bit
        split.checks()
        assert np.array_equal(bits(v0), bits(v1)) and np.array_equal(loss0.view(np.uint64), loss1.view(np.uint64))
        r32, r64 = (fit_grad_reference(p, ft, t_in, w_in, v1, acts) for p in (p32, p64))
        worst = max(worst, check(f"fit grad {what} weights={name}", grad, r32, r64))
        sgd_call(split.mlp, f32(grad), None, ALPHA)
        assert np.array_equal(bits(split.theta()), bits(plain.theta())), (what, name)
        assert same_bits(split.w1t, plain.w1t) and same_bits(split.w1, plain.w1)
        assert not np.array_equal(bits(plain.theta()), bits(theta0))
        split.checks()
    print(f"fit grad {what}: worst ratio {worst:.2f} E")


# ------------------------------------------------------------------ 4: Adam on given gradients
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip1"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("H", [1, 17, 80, 128])
def test_adam_on_given_gradients_against_float64(H, wd, clip):
    cpu = make_net(H, "sigmoid", "tanh", seed=H)
    raw = RawNet(cpu, DEV, 4)
    rows = 200 * H + 1
    grads = R.synthetic_grads(rows, STEPS, 100 + H, 3, ZERO_STEP)
    theta0 = raw.theta()
    refs = [R.Adam(theta0, weight_decay=wd, dtype=dt, **HYPER) for dt in (np.float32, np.float64)]
    m, s = guarded(rows), guarded(rows)
    m[:rows], s[:rows] = 0.0, 0.0
    state = torch.zeros(3, dtype=torch.int64, device=DEV)
    worst = 0.0
    for k in range(STEPS):
        g = f32(grads[k])
        out, c32, c64 = None, None, None
        if clip is not None:
            out = norm_call(H, g, clip)
            c32, c64 = R.clip(grads[k], clip, np.float32), R.clip(grads[k], clip, np.float64)
        adam_call(raw.mlp, g, None if out is None else out[1:], m, s, state, wd)
        for ref, c in zip(refs, (c32, c64)):
            ref.step(grads[k], scale=None if c is None else c[1])
        if k + 1 in (1, 3):
            what = f"H={H} wd={wd} clip={clip} step {k + 1}"
            for key, got in (("theta", raw.theta()), ("m", np_(m[:rows])), ("s", np_(s[:rows]))):
                worst = max(worst, check(f"{key} {what}", got, getattr(refs[0], key), getattr(refs[1], key)))
            if clip is not None:
                o = np_(out)
                worst = max(worst, check(f"norm {what}", o[:1], c32[0], c64[0]), check(f"scale {what}", o[1:], c32[1], c64[1]))
            raw.checks()  # the mirror is the transpose bit for bit, the padding untouched
    assert (m[rows:] == SENT).all() and (s[rows:] == SENT).all()
    assert int(state[0]) == STEPS
    pows = np_(state[1:]).view(np.float64)
    assert abs(pows[0] - R.h(0.9) ** 3) < 1e-15 and abs(pows[1] - R.h(0.999) ** 3) < 1e-15
    assert np.abs(raw.theta() - theta0).max() > 100 * np.spacing(np.float32(np.abs(theta0).max()))  # it moved
    print(f"adam H={H} wd={wd} clip={clip}: worst ratio {worst:.2f} E")


# ------------------------------------------------------------------ 5: the norm and the scale
@pytest.mark.parametrize("H", [1, 17, 128])
def test_norm_and_scaled_steps(H):
    cpu = make_net(H, "tanh", "none", seed=H + 1)
    rows = 200 * H + 1
    grads = R.synthetic_grads(rows, STEPS, 200 + H, 3, ZERO_STEP)
    alpha = 1e-3
    for k in (0, ZERO_STEP):
        g, gd = grads[k], f32(grads[k])
        n64 = float(R.clip(g, 1.0, np.float64)[0])
        for max_norm in (0.0, 1.0, n64 * 0.5, n64 * 4 + 1.0):
            out = norm_call(H, gd, max_norm)
            o = np_(out)
            c32, c64 = R.clip(g, max_norm, np.float32), R.clip(g, max_norm, np.float64)
            what = f"H={H} step {k} max_norm={max_norm:.3g}"
            check(f"norm {what}", o[:1], c32[0], c64[0])
            check(f"scale {what}", o[1:], c32[1], c64[1])
            if max_norm > n64:
                assert o[1] == 1.0  # exactly
            elif n64 > 0:
                assert o[1] < 1.0
            # SGD under the scale: the reference's step; unclipped: the plain step's bits
            clipped, plain = RawNet(cpu, DEV, 4), RawNet(cpu, DEV, 4)
            theta0 = plain.theta()
            sgd_call(clipped.mlp, gd, out[1:], alpha)
            sgd_call(plain.mlp, gd, None, alpha)
            r32, r64 = (R.sgd(theta0, g, alpha, dt, scale=c[1]) for dt, c in ((np.float32, c32), (np.float64, c64)))
            check(f"sgd theta {what}", clipped.theta(), r32, r64)
            clipped.checks()
            if o[1] == 1.0:
                assert np.array_equal(bits(clipped.theta()), bits(plain.theta()))
                assert same_bits(clipped.w1, plain.w1)
            elif n64 > 0 and max_norm > 0:
                assert not np.array_equal(bits(clipped.theta()), bits(plain.theta()))
            if k == ZERO_STEP or max_norm == 0.0:
                assert np.array_equal(bits(clipped.theta()), bits(theta0))
            # Adam under a scale of exactly 1: the unclipped step's bits
            if o[1] == 1.0:
                a, b = RawNet(cpu, DEV, 4), RawNet(cpu, DEV, 4)
                st = [(torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV),
                       torch.zeros(3, dtype=torch.int64, device=DEV)) for _ in range(2)]
                adam_call(a.mlp, gd, out[1:], *st[0], 0.01)
                adam_call(b.mlp, gd, None, *st[1], 0.01)
                assert np.array_equal(bits(a.theta()), bits(b.theta()))
                assert all(same_bits(x, y) for x, y in zip(st[0], st[1]))


# ------------------------------------------------------------------ 6: determinism and the graph
def window_learner(rules, hook=None, optimizer="adam", alpha=None):
    from gym_narde.td import ValueAdam, ValueSGD, WindowTDLambdaLearner

    env = middle_game(rules, 65, max_steps=48, seed=11)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=9)).to(env.device)
    opt = {"adam": lambda: ValueAdam(net, 1e-3, weight_decay=0.01, max_grad_norm=1.0),
           "sgd": lambda: ValueSGD(net, 0.02), None: lambda: None}[optimizer]()
    return WindowTDLambdaLearner(env, net, alpha, lam=0.7, plies=3, gamma=0.95, epsilon=0.1, seed=3, optimizer=opt,
                                 grad_hook=hook)


def lookahead_learner(rules):
    from gym_narde.td import LookaheadTargetLearner, ValueAdam

    env = middle_game(rules, 65, max_steps=48, seed=11)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=9)).to(env.device)
    opt = ValueAdam(net, 1e-3, max_grad_norm=1.0)
    return LookaheadTargetLearner(env, net, None, plies=3, epsilon=0.1, seed=3, optimizer=opt)


def learner_bits(learner):
    opt = learner.optimizer if hasattr(learner, "optimizer") else learner.fitter.optimizer
    out = [p.detach().clone() for p in learner.net.parameters()] + [learner.net._w1t.clone()]
    out += [opt.m.clone(), opt.s.clone(), opt.state.clone(), opt.norm.clone()]
    out += [v.clone() for v in learner.bufs.values()] + list(learner.env.get_state().values())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("make,rules", [(window_learner, "ref2"), (lookahead_learner, "full4")],
                         ids=["window-ref2", "lookahead-full4"])
def test_same_seed_same_bits_and_graph_replays_three_steps(make, rules):
    """Four eager steps run twice give the same bits; and with steps 2 to 4 as
    one captured step replayed three times, the device's step count included."""
    runs = []
    for graphed in (False, False, True):
        learner = make(rules)
        learner.step()  # the device has seen one call
        torch.cuda.synchronize()
        if not graphed:
            for _ in range(3):
                learner.step()
        else:
            before = learner_bits(learner)
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    learner.step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            for a, b in zip(learner_bits(learner), before):  # capture ran nothing
                assert same_bits(a, b)
            for _ in range(3):
                graph.replay()
        runs.append(learner_bits(learner))
        opt = learner.optimizer if hasattr(learner, "optimizer") else learner.fitter.optimizer
        assert int(opt.steps) == 4 and opt.steps.is_cuda
        learner.env.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert same_bits(a, b)
    assert not torch.equal(runs[0][0].cpu(), make_net(80, "sigmoid", "tanh", seed=9).l1.weight.detach())  # it did learn
    assert torch.equal(runs[0][4].view(torch.int32), runs[0][0].t().contiguous().view(torch.int32))  # _w1t = the mirror


# ------------------------------------------------------------------ 7: the state's round trip
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_state_round_trip(kind):
    from gym_narde.td import ValueAdam, ValueSGD

    H = 17
    rows = 200 * H + 1
    grads = [f32(g) for g in R.synthetic_grads(rows, STEPS, 7, 3, ZERO_STEP)]
    make = (lambda net: ValueAdam(net, 1e-3, weight_decay=0.01, max_grad_norm=1.0)) if kind == "adam" else \
        (lambda net: ValueSGD(net, 1e-3, max_grad_norm=1.0))
    net_a = copy.deepcopy(make_net(H, "sigmoid", "tanh", seed=2)).to(DEV)
    opt_a = make(net_a)
    for g in grads[:2]:
        opt_a.step(g)
    torch.cuda.synchronize()
    saved = {k: v.cpu() for k, v in opt_a.state_dict().items()}  # as a file would hold it
    net_b = copy.deepcopy(net_a)
    assert net_b._w1t is not net_a._w1t
    opt_b = make(net_b)
    opt_b.load_state_dict(saved)
    opt_a.step(grads[2])
    opt_b.step(grads[2])
    torch.cuda.synchronize()
    assert int(opt_a.steps) == int(opt_b.steps) == 3
    for a, b in zip(list(net_a.parameters()) + [net_a._w1t], list(net_b.parameters()) + [net_b._w1t]):
        assert same_bits(a.detach(), b.detach())
    for key, val in opt_a.state_dict().items():
        assert same_bits(val, opt_b.state_dict()[key]), key
    assert torch.equal(net_a._w1t.view(torch.int32), net_a.l1.weight.detach().t().contiguous().view(torch.int32))
    assert opt_a.memory_bytes() >= (8 * rows if kind == "adam" else 8)
    with pytest.raises(ValueError, match="expected"):
        opt_b.load_state_dict({k: v[..., None] for k, v in saved.items()})


# ------------------------------------------------------------------ 8: the hook
def test_hook_sees_the_learners_gradient():
    seen = []

    def zero(g):
        seen.append((tuple(g.shape), g.dtype, g.device.type))
        g.zero_()

    learner = window_learner("ref2", hook=zero, optimizer="sgd")
    before = [p.detach().clone() for p in learner.net.parameters()] + [learner.net._w1t.clone()]
    for _ in range(2):
        learner.step()
    torch.cuda.synchronize()
    P = 200 * 80 + 1
    assert seen == [((P,), torch.float32, "cuda")] * 2  # once a step
    for a, b in zip(before, list(learner.net.parameters()) + [learner.net._w1t]):
        assert same_bits(a, b.detach())  # a zeroed gradient leaves every weight bit
    assert int(learner.optimizer.steps) == 2
    learner.env.close()

    kept = []

    def double(g):
        kept.append(g.clone())
        g.mul_(2.0)

    learner = window_learner("ref2", hook=double, optimizer="sgd")
    theta0 = T.theta_row(T.params_of(learner.net, torch.float32, "cpu")).numpy()
    learner.play()
    g_alone = learner.gradient().clone()  # moves no weight
    torch.cuda.synchronize()
    assert np.array_equal(bits(T.theta_row(T.params_of(learner.net, torch.float32, "cpu")).numpy()), bits(theta0))
    learner.update()
    torch.cuda.synchronize()
    assert len(kept) == 1 and same_bits(kept[0], g_alone) and float(g_alone.abs().max()) > 0
    got = T.theta_row(T.params_of(learner.net, torch.float32, "cpu")).numpy()
    r32, r64 = (R.sgd(theta0, np_(kept[0]), 2 * 0.02, dt) for dt in (np.float32, np.float64))
    print(f"doubled gradient against alpha * 2: {check('theta doubled', got, r32, r64):.2f} E")
    assert not np.array_equal(bits(got), bits(theta0))
    learner.env.close()


# ------------------------------------------------------------------ 9: learning
def test_adam_fits_lower_the_loss_on_known_outcomes():
    """test_gpu_value_fit's 64 positions one roll from the end, whose playout
    targets are the winner's points: 10 Adam steps lower the squared error."""
    from gym_narde.td import ValueAdam, ValueFitter
    from gym_narde.vector import VecNardeEnv

    B, trials = 64, 4
    board, off = np.zeros((B, 24), np.int8), np.zeros((B, 2), np.uint8)
    player = np.where(np.arange(B) % 2 == 0, 1, -1).astype(np.int8)
    for j in range(B):
        k = (j // 2) % 13
        if player[j] == 1:
            board[j, 0], board[j, 14], off[j] = 1, -(15 - k), (14, k)
        else:
            board[j, 12], board[j, 2], off[j] = -1, 15 - k, (k, 14)
    env = VecNardeEnv(1, device=DEV, seed=1)
    net = copy.deepcopy(make_net(40, "sigmoid", "none", seed=3, scale=1.0)).to(env.device)
    roots = env.state_records(board, off, np.zeros((B, 2), np.uint8), player)
    res = env.playout(roots, trials, net, max_plies=4, seed=9)
    target, weight = env.playout_targets(res, roots=roots)
    fit = ValueFitter(env, net, B, optimizer=ValueAdam(net, 1e-3))
    first = fit.evaluate(roots, target, weight).clone()
    w0 = net.l1.weight.detach().clone()
    g = fit.gradient(roots, target, weight).clone()
    torch.cuda.synchronize()
    assert torch.equal(w0, net.l1.weight.detach()) and float(g.abs().max()) > 0  # gradient() moves no weight
    for _ in range(10):
        loss = fit.step(roots, target, weight)
    last = fit.evaluate(roots, target, weight).clone()
    torch.cuda.synchronize()
    assert loss is fit.loss and int(fit.optimizer.steps) == 10
    a, b = float(first[0] / first[1]), float(last[0] / last[1])
    print(f"mean squared error: first {a:.4f}, after 10 Adam steps {b:.4f}")
    assert b < a
    env.close()


# ------------------------------------------------------------------ 10: the Python errors
def test_optimisers_and_learners_refuse_what_they_cannot_run():
    from gym_narde.td import (LookaheadTargetLearner, PlayoutTargetLearner, ValueAdam, ValueFitter, ValueSGD,
                              WindowTDLambdaLearner)
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device=DEV, seed=1)
    cpu = make_net(16, "sigmoid", "tanh", seed=1)
    with pytest.raises(ValueError, match="GPU"):
        ValueAdam(cpu, 1e-3)  # the net is on the CPU
    with pytest.raises(TypeError):
        ValueSGD(torch.nn.Linear(198, 1).to(DEV), 0.1)
    net, other = copy.deepcopy(cpu).to(DEV), copy.deepcopy(cpu).to(DEV)
    for bad in (dict(lr=-1.0), dict(lr=1e-3, betas=(1.0, 0.999)), dict(lr=1e-3, betas=(0.9, -0.1)), dict(lr=1e-3, eps=0.0),
                dict(lr=1e-3, weight_decay=-0.1), dict(lr=1e-3, max_grad_norm=-1.0), dict(lr=float("nan"))):
        with pytest.raises(ValueError):
            ValueAdam(net, **bad)
    for bad in (dict(alpha=-0.1), dict(alpha=0.1, max_grad_norm=-2.0)):
        with pytest.raises(ValueError):
            ValueSGD(net, **bad)
    opt = ValueAdam(net, 1e-3)
    with pytest.raises(ValueError, match="grad must be"):
        opt.step(torch.zeros(5, device=DEV))
    with pytest.raises(ValueError, match="grad must be"):
        opt.step(torch.zeros(200 * 16 + 1))  # on the CPU
    with pytest.raises(ValueError, match="another net"):
        WindowTDLambdaLearner(env, other, None, lam=0.5, plies=4, optimizer=opt)
    with pytest.raises(ValueError, match="mutually exclusive"):
        WindowTDLambdaLearner(env, net, 0.1, lam=0.5, plies=4, optimizer=opt)
    with pytest.raises(ValueError, match="mutually exclusive"):
        PlayoutTargetLearner(env, net, 0.1, plies=4, trials=2, optimizer=opt)
    with pytest.raises(ValueError, match="mutually exclusive"):
        LookaheadTargetLearner(env, net, 0.1, plies=4, optimizer=opt)
    with pytest.raises(ValueError, match="alpha or an optimizer"):
        WindowTDLambdaLearner(env, net, None, lam=0.5, plies=4)
    with pytest.raises(ValueError, match="grad_hook needs an optimizer"):
        WindowTDLambdaLearner(env, net, 0.1, lam=0.5, plies=4, grad_hook=lambda g: None)
    with pytest.raises(TypeError, match="ValueSGD or ValueAdam"):
        ValueFitter(env, net, 8, optimizer=torch.optim.SGD(net.parameters(), lr=0.1))
    st = env.get_state()
    records = env.state_records(st["board"], st["off"], st["first_turn"], st["player"])
    fit = ValueFitter(env, net, 8, optimizer=opt)
    with pytest.raises(ValueError, match="mutually exclusive"):
        fit.step(records, torch.zeros(8), alpha=0.1)
    with pytest.raises(TypeError, match="alpha"):
        ValueFitter(env, net, 8).step(records, torch.zeros(8))
    if torch.cuda.device_count() > 1:
        far = VecNardeEnv(8, device="cuda:1", seed=1)
        with pytest.raises(ValueError):
            ValueFitter(far, net, 8, optimizer=opt)
        far.close()
    env.close()


# ------------------------------------------------------------------ 11: the example
def test_the_training_example_trains_with_adam_and_its_file_loads(tmp_path):
    from gym_narde.value_net import ValueMLP

    out = tmp_path / "agent.pt"
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "train_value_agent.py"),
           "--window", "4", "--envs", "64", "--plies", "12", "--optimizer", "adam", "--lr", "1e-3", "--clip", "1",
           "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "saved" in res.stdout and "adam" in res.stdout
    net = ValueMLP(80, "sigmoid", "tanh")
    net.load_state_dict(torch.load(out, map_location="cpu"))
    assert all(torch.isfinite(p).all() for p in net.parameters())  # what play_value_agent.py --weights loads
