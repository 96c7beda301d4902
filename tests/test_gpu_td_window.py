"""Windowed TD(lambda) on the GPU: the records the
one-launch rollouts write (narde_value_rollout_records,
narde_turn_value_rollout_records), narde_value_td_window
(kernels_td_window.h) and gym_narde.td.WindowTDLambdaLearner.

Reference for the update: narde.h's semantics in torch float64
(test_td_window_cpu.reference: td_ref.value_and_grad, td_targets, the backward
recursion for G) on O.tesauro198 rows of the recorded states.  Tolerance:
8 x E, E = max |the same formulas in float32 - float64| per compared array,
floored at one float32 ulp of its largest magnitude -- td_ref's rule, never a
figure of the code under test.
"""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import td_ref as T
from conftest import ROOT
from test_afterstates_cpu import golden_states
from test_td_window_cpu import ALPHA, GAMMA, reference
from test_value_cpu import make_net
from test_value_rollout_cpu import endgames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import np_  # noqa: E402

SENT = -7.25  # what padding holds before and after
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ records
def pack_record(st, t):
    """The 32-byte records (B, 8) int32 of get_state()'s dict and the ply
    counter t, as narde_rules.h lays them out: p0 = {white w0, w1, black w0,
    w1}, p1 = {white w2, black w2, misc, t}, a nibble a point."""
    board = np_(st["board"]).astype(np.int64)
    off, ft = np_(st["off"]).astype(np.int64), np_(st["first_turn"]).astype(np.int64)
    player, elapsed = np_(st["player"]).astype(np.int64), np_(st["elapsed"]).astype(np.int64) & 0xFFFF
    w, k = np.clip(board, 0, None), np.clip(-board, 0, None)
    sh = 4 * (np.arange(24) % 8)
    word = lambda c, i: ((c[:, 8 * i:8 * i + 8] << sh[:8]).sum(1))  # noqa: E731
    misc = off[:, 0] | (off[:, 1] << 4) | (ft[:, 0] << 8) | (ft[:, 1] << 9) | ((player == -1).astype(np.int64) << 10) | (elapsed << 16)
    rec = np.stack([word(w, 0), word(w, 1), word(k, 0), word(k, 1), word(w, 2), word(k, 2), misc,
                    np.full(len(player), int(t), np.int64)], 1)
    return (rec & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def unpack_record(rec):
    """(board int8 (n, 24), off uint8 (n, 2), player int8 (n,)) of records (n, 8)."""
    r = np.ascontiguousarray(rec).view(np.uint32).astype(np.int64)
    sh = 4 * np.arange(8)
    nib = lambda x: (x[:, None] >> sh) & 15  # noqa: E731
    w = np.concatenate([nib(r[:, 0]), nib(r[:, 1]), nib(r[:, 4])], 1)
    k = np.concatenate([nib(r[:, 2]), nib(r[:, 3]), nib(r[:, 5])], 1)
    misc = r[:, 6]
    off = np.stack([misc & 15, (misc >> 4) & 15], 1).astype(np.uint8)
    return (w - k).astype(np.int8), off, np.where((misc >> 10) & 1, -1, 1).astype(np.int8)


def three_envs(rules, B, max_steps, state):
    from gym_narde.vector import VecNardeEnv

    envs = [VecNardeEnv(B, device=DEV, seed=23, rules=rules, max_episode_steps=max_steps) for _ in range(3)]
    for env in envs:
        if state is None:
            env.selfplay(30)
        else:
            env.set_state(*state)
    return envs


RECORD_CASES = [(rules, B, plies, None) for rules in ("ref2", "full4") for B in (1, 65) for plies in (1, 7)]
RECORD_CASES += [(rules, 65, 7, kind) for rules in ("ref2", "full4") for kind in ("epsilon", "max_steps")]
RECORD_CASES += [(rules, 8, 3, "endgame") for rules in ("ref2", "full4")]


@pytest.mark.parametrize("rules,B,plies,kind", RECORD_CASES, ids=lambda x: str(x))
def test_records_are_the_stepped_envs_records(rules, B, plies, kind):
    state = None
    if kind == "endgame":
        b, o, f, p = endgames()  # one ply from winning: both colours, 1 and 2 points
        state = tuple(np.ascontiguousarray(np.concatenate([a, a])) for a in (b, o, f, p))
    rec_env, parent, loop = three_envs(rules, B, 5 if kind == "max_steps" else 1000, state)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=5)).to(rec_env.device)
    kw = dict(epsilon=0.3, tag=11, seed=9) if kind == "epsilon" else {}
    full = rules == "full4"
    run = (lambda env, bufs: env.turn_value_rollout(plies, net, bufs=bufs, **kw)) if full else \
        (lambda env, bufs: env.value_rollout(plies, net, bufs=bufs, **kw))
    make = (lambda env, **k: env.turn_value_rollout_buffers(plies, **k)) if full else \
        (lambda env, **k: env.value_rollout_buffers(plies, **k))
    assert "records" not in make(parent)  # the default is the parent's dict
    got = run(rec_env, make(rec_env, records=True))
    want = run(parent, make(parent))
    torch.cuda.synchronize()
    # every other output and the final state: the parent call's
    for name, a in want.items():
        assert torch.equal(got[name].view(torch.uint8), a.view(torch.uint8)), name
    sa, sb = rec_env.get_state(), parent.get_state()
    assert all(torch.equal(sa[key], sb[key]) for key in sa) and torch.equal(rec_env.stats(), parent.stats())
    assert rec_env.ply == parent.ply
    # records[k]: a second env stepped with the launch's plays and dice
    records = np_(got["records"])
    column = got["play" if full else "actions"]
    for k in range(plies):
        assert np.array_equal(records[k], pack_record(loop.get_state(), loop.ply)), f"ply {k}"
        loop.step(column[k], got["dice"][k])
    torch.cuda.synchronize()
    sc = loop.get_state()
    assert all(torch.equal(sa[key], sc[key]) for key in sa)
    term, trunc = np_(got["terminated"]).astype(bool), np_(got["truncated"]).astype(bool)
    if kind == "endgame":
        assert term[0].all() and plies > 1  # the terminal pick and its reset fall inside the window
    if kind == "max_steps":
        assert trunc.any() and trunc[:-1].any()
    for env in (rec_env, parent, loop):
        env.close()


def test_records_buffer_is_checked():
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device=DEV, seed=1)
    net = make_net(16, "sigmoid", "tanh", seed=1).to(env.device)
    bufs = env.value_rollout_buffers(3, records=True)
    assert bufs["records"].shape == (3, 8, 8) and bufs["records"].dtype == torch.int32
    bufs["records"] = bufs["records"][:, :, :4].contiguous()
    with pytest.raises(ValueError, match="records"):
        env.value_rollout(3, net, bufs=bufs)
    env.close()


# ------------------------------------------------- narde_value_td_window
class RawNet:
    """A ValueMLP's weights in padded device arrays of their own, the padding
    full of SENT: ld_w1t = hidden + pad, ld_w1 = 198 + 2."""

    def __init__(self, cpu, dev, pad=0):
        from gym_narde import _lib
        from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

        H = cpu.hidden
        self.H, self.ld, self.ld_w1 = H, H + pad, 200
        f = dict(dtype=torch.float32, device=dev)
        self.w1t = torch.full((198, self.ld), SENT, **f)
        self.w1t[:, :H] = cpu.l1.weight.detach().t().to(dev)
        self.w1 = torch.full((H, self.ld_w1), SENT, **f)
        self.w1[:, :198] = cpu.l1.weight.detach().to(dev)
        self.b1 = cpu.l1.bias.detach().clone().to(dev)
        self.w2 = cpu.l2.weight.detach().reshape(-1).clone().to(dev)
        self.b2 = cpu.l2.bias.detach().clone().to(dev)
        self.mlp = _lib.ValueMlpTrain(self.w1t.data_ptr(), self.ld, self.b1.data_ptr(), self.w2.data_ptr(),
                                      self.b2.data_ptr(), H, HIDDEN_ACTS[cpu.hidden_act], OUT_ACTS[cpu.out_act],
                                      self.w1.data_ptr(), self.ld_w1)

    def params(self, dtype):
        c = lambda x: x.detach().cpu().to(dtype)  # noqa: E731
        return c(self.w1t[:, :self.H]).t().contiguous(), c(self.b1), c(self.w2), c(self.b2).reshape(())

    def theta(self):
        return T.theta_row(self.params(torch.float32)).numpy()

    def checks(self):
        assert (self.w1t[:, self.H:] == SENT).all() and (self.w1[:, 198:] == SENT).all()
        assert torch.equal(self.w1[:, :198].view(torch.int32), self.w1t[:, :self.H].t().contiguous().view(torch.int32))


def window_call(env, mlp, plies, bufs, alpha, lam, gamma, H):
    """narde_value_td_window on a launch's buffers: (v (K + 1, B), delta (K, B))."""
    from gym_narde import _lib

    B = env.num_envs
    n = _lib.td_window_scratch_floats(B, plies, H)
    scratch = torch.full((n + 4,), SENT, dtype=torch.float32, device=env.device)
    delta = torch.full((plies, B), SENT, dtype=torch.float32, device=env.device)
    env.handle.call("narde_value_td_window", ctypes.byref(mlp), plies, _lib.ptr(bufs["records"]),
                    _lib.ptr(bufs["reward"]), _lib.ptr(bufs["terminated"]), _lib.ptr(bufs["truncated"]), alpha, lam,
                    gamma, _lib.ptr(scratch), n, _lib.ptr(delta), env._s())
    torch.cuda.synchronize()
    assert (scratch[n:] == SENT).all()
    return scratch[:(plies + 1) * B].view(plies + 1, B), delta


def window_inputs(bufs, env, plies):
    """(feat ((K + 1) B, 198), player, reward, term, trunc) of a launch's
    buffers and the env's state as it stands."""
    B = env.num_envs
    board, off, player = unpack_record(np_(bufs["records"])[:plies].reshape(plies * B, 8))
    st = env.get_state()
    board = np.concatenate([board, np_(st["board"])])
    off = np.concatenate([off, np_(st["off"])])
    player = np.concatenate([player, np_(st["player"])])
    return (O.tesauro198(board, off, player), player, np_(bufs["reward"])[:plies], np_(bufs["terminated"])[:plies],
            np_(bufs["truncated"])[:plies])


def compare(what, got, r32, r64):
    """got, r32, r64: (v, delta, theta) each; the worst ratio."""
    worst = 0.0
    for name, g, a, b in zip(("v", "delta", "theta"), got, r32, r64):
        bd = T.Bound(f"{name} {what}")
        bd.add(np_(g) if torch.is_tensor(g) else g, a.numpy(), b.numpy())
        worst = max(worst, bd.check())
    return worst


def middle_game(rules, B, max_steps=44, seed=7):
    """B envs 40 plies into self-play, the elapsed counts staggered so that
    the TimeLimit falls inside a window, and (B >= 8) eight envs one ply from
    winning."""
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(B, device=DEV, seed=seed, rules=rules, max_episode_steps=max_steps)
    env.selfplay(40)
    st = {k: v.clone() for k, v in env.get_state().items()}
    st["elapsed"] = (torch.arange(B, device=env.device) % 4 + max_steps - 4).to(torch.int16)
    if B >= 16:
        b, o, f, p = endgames()
        for key, a in (("board", b), ("off", o), ("first_turn", f), ("player", p)):
            st[key][8:16] = torch.as_tensor(np.concatenate([a, a])).to(env.device)
        st["elapsed"][8:16] = 3
    env.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"])
    return env


WINDOW_CASES = [(1, 1, 80, "sigmoid", "tanh", "ref2", 0), (1, 7, 1, "relu", "none", "full4", 0),
                (1, 2, 128, "tanh", "none", "ref2", 0), (63, 2, 17, "sigmoid", "none", "ref2", 0),
                (63, 7, 128, "tanh", "sigmoid", "full4", 0), (63, 1, 1, "relu", "tanh", "ref2", 0),
                (65, 1, 128, "tanh", "tanh", "full4", 0), (65, 2, 80, "relu", "sigmoid", "ref2", 0),
                (65, 7, 17, "sigmoid", "tanh", "ref2", 0), (65, 7, 80, "sigmoid", "sigmoid", "full4", 0),
                (65, 7, 80, "sigmoid", "tanh", "ref2", 4)]


@pytest.mark.parametrize("B,plies,H,hact,oact,rules,pad", WINDOW_CASES, ids=lambda x: str(x))
def test_window_update_against_float64(B, plies, H, hact, oact, rules, pad):
    env = middle_game(rules, B)
    cpu = make_net(H, hact, oact, seed=H + plies)
    net = copy.deepcopy(cpu).to(env.device)
    make = env.turn_value_rollout_buffers if env.full else env.value_rollout_buffers
    bufs = make(plies, records=True)
    (env.turn_value_rollout if env.full else env.value_rollout)(plies, net, epsilon=0.2, tag=0, seed=4, bufs=bufs)
    raw = RawNet(cpu, env.device, pad)
    p32, p64 = raw.params(torch.float32), raw.params(torch.float64)
    lam = 0.7
    v, delta = window_call(env, raw.mlp, plies, bufs, ALPHA, lam, GAMMA, H)
    feat, player, reward, term, trunc = window_inputs(bufs, env, plies)
    if B == 65 and plies == 7:  # the window holds what it was built to hold
        assert term.any() and trunc.any() and ((term | trunc) == 0).sum() > B
    refs = [reference(p, feat, player, reward, term, trunc, plies, B, lam, hact, oact) for p in (p32, p64)]
    pick = lambda r: (r[0], r[1], r[3])  # noqa: E731
    what = f"B={B} K={plies} H={H} {hact}/{oact} {rules} pad={pad}"
    worst = compare(what, (v, delta, raw.theta()), pick(refs[0]), pick(refs[1]))
    print(f"{what}: worst ratio {worst:.2f} E")
    d = np_(delta)
    assert (d[(trunc == 1) & (term == 0)] == 0).all()
    moved = float((refs[1][3] - T.theta_row(p64)).abs().max())
    assert moved > 10 * T.TOL_FACTOR * float(np.spacing(np.float32(refs[1][3].abs().max())))  # a lost update would show
    raw.checks()
    env.close()


def test_one_ply_window_is_the_online_learners_update():
    """plies = 1, lam = 0, greedy: trace(decay 0) + step + apply from the same
    state and weights.  The summation order differs (slabs of 64 envs there,
    of 128 samples here): within 8 E of each other, E the float64
    reference's own."""
    from gym_narde.td import TDLambdaLearner, WindowTDLambdaLearner

    B, alpha, gamma, acts = 65, 0.05, 0.9, ("sigmoid", "tanh")
    cpu = make_net(80, *acts, seed=12)
    env_a, env_b = middle_game("ref2", B), middle_game("ref2", B)
    net_a, net_b = copy.deepcopy(cpu).to(env_a.device), copy.deepcopy(cpu).to(env_a.device)
    online = TDLambdaLearner(env_a, net_a, alpha=alpha, lam=0.0, gamma=gamma)
    window = WindowTDLambdaLearner(env_b, net_b, alpha=alpha, lam=0.0, plies=1, gamma=gamma)
    p32, p64 = T.params_of(net_b, torch.float32, "cpu"), T.params_of(net_b, torch.float64, "cpu")
    out = online.step()
    reward, term, trunc, delta = window.step()
    torch.cuda.synchronize()
    assert torch.equal(out[1], reward[0]) and torch.equal(out[2], term[0]) and torch.equal(out[3], trunc[0])
    sa, sb = env_a.get_state(), env_b.get_state()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    feat, player, rw, tm, tr = window_inputs(window.bufs, env_b, 1)

    def theta_of(p, dt):
        x = torch.from_numpy(feat).to(dt)
        v, grad = T.value_and_grad(p, x, *acts)
        d = T.td_targets(v[:B], v[B:], torch.from_numpy(rw[0]), torch.from_numpy(player[:B] == -1),
                         torch.from_numpy(tm[0]), torch.from_numpy(tr[0]), torch.tensor(gamma, dtype=dt))
        return d, T.theta_row(p) + torch.tensor(alpha, dtype=dt) * (d[:, None] * grad[:B]).sum(0)

    (d32, t32), (d64, t64) = theta_of(p32, torch.float32), theta_of(p64, torch.float64)
    got_w = T.theta_row(T.params_of(net_b, torch.float32, "cpu")).numpy()
    got_o = T.theta_row(T.params_of(net_a, torch.float32, "cpu")).numpy()
    for what, g in (("window", got_w), ("online", got_o)):
        bd = T.Bound(f"theta {what}")
        bd.add(g, t32.numpy(), t64.numpy())
        bd.check()
    e = T.error_bound(t32.numpy(), t64.numpy())
    gap = float(np.abs(got_w.astype(np.float64) - got_o.astype(np.float64)).max())
    print(f"window against online: {gap:.3e} = {gap / e:.2f} E")
    assert gap <= T.TOL_FACTOR * e
    bd = T.Bound("delta window against online")
    bd.add(np_(delta[0]), d32.numpy(), d64.numpy())
    bd.check()
    gap = float(np.abs(np_(delta[0]).astype(np.float64) - np_(out[-1]).astype(np.float64)).max())
    assert gap <= T.TOL_FACTOR * T.error_bound(d32.numpy(), d64.numpy())
    env_a.close()
    env_b.close()


# ------------------------------------------------- WindowTDLambdaLearner
def make_learner(rules, lam, seed=3, B=65, plies=3, alpha=0.02, gamma=0.95):
    from gym_narde.td import WindowTDLambdaLearner

    env = middle_game(rules, B, max_steps=48, seed=11)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=9)).to(env.device)
    return WindowTDLambdaLearner(env, net, alpha=alpha, lam=lam, plies=plies, gamma=gamma, epsilon=0.1, seed=seed)


def reference_step(p, feat, player, reward, term, trunc, K, B, lam, alpha, gamma, acts):
    """narde.h's semantics in p's dtype: (v, delta, theta)."""
    dt = p[0].dtype
    v, grad = T.value_and_grad(p, torch.from_numpy(feat).to(dt), *acts)
    v = v.reshape(K + 1, B)
    tm, tr = torch.from_numpy(term), torch.from_numpy(trunc)
    delta = T.td_targets(v[:K], v[1:], torch.from_numpy(reward), torch.from_numpy((player[:K * B] == -1).reshape(K, B)),
                         tm, tr, torch.tensor(gamma, dtype=dt))
    c = torch.where((tm | tr).bool(), torch.zeros((), dtype=dt), torch.tensor(gamma, dtype=dt) * torch.tensor(lam, dtype=dt))
    G, nxt = torch.zeros_like(delta), torch.zeros(B, dtype=dt)
    for k in range(K - 1, -1, -1):
        nxt = delta[k] + c[k] * nxt
        G[k] = nxt
    return v, delta, T.theta_row(p) + torch.tensor(alpha, dtype=dt) * (G.reshape(-1, 1) * grad[:K * B]).sum(0)


@pytest.mark.parametrize("lam", [0.0, 0.7])
@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_ten_learner_steps_teacher_forced(rules, lam):
    """Each step's reference starts from the GPU's own weights of the step
    before, so rounding does not compound."""
    learner = make_learner(rules, lam)
    env, net, K, B = learner.env, learner.net, learner.plies, learner.env.num_envs
    acts = (net.hidden_act, net.out_act)
    assert learner.memory_bytes() >= 4 * learner.scratch.numel() + 32 * K * B
    worst, ended = 0.0, 0
    for step in range(10):
        p32, p64 = T.params_of(net, torch.float32, "cpu"), T.params_of(net, torch.float64, "cpu")
        reward, term, trunc, delta = learner.step()
        torch.cuda.synchronize()
        assert reward.shape == term.shape == trunc.shape == delta.shape == (K, B)
        feat, player, rw, tm, tr = window_inputs(learner.bufs, env, K)
        ended += int((tm | tr).sum())
        r32, r64 = (reference_step(p, feat, player, rw, tm, tr, K, B, lam, learner.alpha, learner.gamma, acts)
                    for p in (p32, p64))
        got = (learner.values(), delta, T.theta_row(T.params_of(net, torch.float32, "cpu")).numpy())
        worst = max(worst, compare(f"{rules} lam={lam} step {step}", got, r32, r64))
        assert torch.equal(net._w1t.view(torch.int32), net.l1.weight.t().contiguous().view(torch.int32))
        assert int(learner._tag) == (step + 1) * K
    assert ended > 0
    print(f"{rules} lam={lam}: worst ratio {worst:.2f} E")
    env.close()


def learner_bits(learner):
    out = [p.detach().clone() for p in learner.net.parameters()] + [learner.net._w1t.clone(), learner.delta.clone()]
    out += [v.clone() for v in learner.bufs.values()] + list(learner.env.get_state().values())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_same_seed_same_bits_and_graph_replay(rules):
    """Four steps run twice give the same bits; and with the fourth step
    captured (launch + update) and replayed once in place of the eager one."""
    runs = []
    for graphed in (False, False, True):
        learner = make_learner(rules, 0.7)
        for _ in range(3):
            learner.step()
        torch.cuda.synchronize()
        if not graphed:
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
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            graph.replay()
        runs.append(learner_bits(learner))
        learner.env.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert not torch.equal(runs[0][0].cpu(), make_net(80, "sigmoid", "tanh", seed=9).l1.weight.detach())  # it did learn


def test_scored_calls_see_the_update_without_pack():
    from gym_narde.td import WindowTDLambdaLearner
    from gym_narde.vector import VecNardeEnv
    from test_gpu_value import check_values, expected

    env = VecNardeEnv(257, device=DEV, seed=8)
    env.selfplay(40)
    net = copy.deepcopy(make_net(80, "sigmoid", "sigmoid", seed=1)).to(env.device)
    before = net.l1.weight.detach().clone()
    learner = WindowTDLambdaLearner(env, net, alpha=0.05, lam=0.7, plies=3)

    def no_pack():
        raise AssertionError("pack() called")

    net.pack = no_pack
    for _ in range(3):
        learner.step()
    assert (net.l1.weight.detach() - before).abs().max() > 1e-3
    plain = env.afterstates()
    aft, values = env.scored_afterstates(net, perspective="white")
    cpu = copy.deepcopy(net).cpu()
    want, E, term = expected(cpu, plain.feat, plain.reward, "white")
    check_values(values, want, E, term, "after three window updates")
    env.close()


def test_learner_refuses_what_it_cannot_run():
    from gym_narde.td import WindowTDLambdaLearner
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device=DEV, seed=1)
    net = make_net(16, "sigmoid", "tanh", seed=1)
    with pytest.raises(ValueError, match="is on"):
        WindowTDLambdaLearner(env, net, alpha=0.1, lam=0.5, plies=4)  # the net is on the CPU
    net = net.to(env.device)
    with pytest.raises(TypeError):
        WindowTDLambdaLearner(env, torch.nn.Linear(198, 1).to(env.device), alpha=0.1, lam=0.5, plies=4)
    fixed = VecNardeEnv(8, device=DEV, seed=1, autoreset=False)
    with pytest.raises(ValueError, match="autoreset"):
        WindowTDLambdaLearner(fixed, net, alpha=0.1, lam=0.5, plies=4)
    with pytest.raises(ValueError, match="lam"):
        WindowTDLambdaLearner(env, net, alpha=0.1, lam=1.5, plies=4)
    with pytest.raises(ValueError, match="plies"):
        WindowTDLambdaLearner(env, net, alpha=0.1, lam=0.5, plies=0)
    learner = WindowTDLambdaLearner(env, net, alpha=0.1, lam=0.5, plies=4)
    from gym_narde import _lib

    per_sample = 2 + 4 + 4 + 4 + 1 + 1 + 32 + 4  # dice, actions, value, reward, terminated, truncated, records, delta
    assert learner.memory_bytes() == 4 * 8 * per_sample + 4 * _lib.td_window_scratch_floats(8, 4, 16)
    fixed.close()
    env.close()


def test_one_ply_windows_learn_a_fixed_regression():
    """test_gpu_td.py's regression restated: 64 one-ply-to-win positions (the
    mover has borne off 14 and both dice bear the last checker off), reset
    every iteration; plies = 1 windows over their records and the step's
    reward and flags, lam 0, linear output: gradient descent of v(s) towards
    the outcomes, so the mean |delta| shrinks."""
    from gym_narde.vector import VecNardeEnv

    board, off, ft, player, dice = (np.asarray(a) for a in golden_states())
    mine = np.where(player[:, None] == 1, board, -np.roll(board, 12, axis=1))
    own = np.clip(mine, 0, None)
    m_off = np.where(player == 1, off[:, 0], off[:, 1])
    last = own.argmax(1)
    sure = np.nonzero((m_off == 14) & (own.sum(1) == 1) & (last <= 5) & (dice.min(1) >= last + 1))[0]
    assert len(sure) >= 16 and {1, -1} <= set(player[sure])
    B = 64
    idx = sure[(np.arange(B) * 5) % len(sure)]
    st = {k: np.ascontiguousarray(a[idx]) for k, a in (("board", board), ("off", off), ("ft", ft), ("player", player),
                                                       ("dice", dice))}
    env = VecNardeEnv(B, device=DEV, seed=1)
    cpu = make_net(40, "sigmoid", "none", seed=3, scale=1.0)
    raw = RawNet(cpu, env.device)
    env.set_state(st["board"], st["off"], st["ft"], st["player"])
    records = torch.from_numpy(pack_record(env.get_state(), env.ply)).to(env.device).reshape(1, B, 8).contiguous()
    errs = []
    for _ in range(31):
        env.set_state(st["board"], st["off"], st["ft"], st["player"])
        _, reward, term, trunc, _ = env.step(None, st["dice"])
        assert bool(term.all())
        bufs = dict(records=records, reward=reward.reshape(1, B), terminated=term.reshape(1, B),
                    truncated=trunc.reshape(1, B))
        _, delta = window_call(env, raw.mlp, 1, bufs, 2e-4, 0.0, 1.0, 40)
        errs.append(float(delta.abs().mean()))
    print(f"mean |delta|: first {errs[0]:.4f}, after 30 windows {errs[-1]:.4f}")
    assert errs[-1] < errs[0]
    raw.checks()
    env.close()


def test_the_training_example_trains_by_windows(tmp_path):
    from gym_narde.value_net import ValueMLP

    out = tmp_path / "agent.pt"
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "train_value_agent.py"),
           "--window", "8", "--envs", "64", "--plies", "24", "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "saved" in res.stdout
    sd = torch.load(out, map_location="cpu")
    net = ValueMLP(80, "sigmoid", "tanh")
    net.load_state_dict(sd)
    assert all(torch.isfinite(p).all() for p in net.parameters())
