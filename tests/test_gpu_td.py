"""TD(lambda) on the value MLP on the GPU (kernels_td.h through
narde_value_td_trace / narde_value_td_apply and gym_narde.td.TDLambdaLearner).

Reference: td_ref's explicit per-sample formulas in float64 on O.tesauro198
rows of the states read back from the env.  Tolerance: 8 x E, E = max |the
same formulas in float32 - float64| per compared array, floored at one
float32 ulp of its largest magnitude (tests/test_td_cpu.py states the
argument) -- never a figure of the code under test.
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
from test_value_cpu import make_net

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import np_  # noqa: E402

SLAB = 64  # NARDE_TD_SLAB: the envs one partial row of the apply pass sums
SENT = -7.25  # what padding holds before and after
MAX_STEPS = 50


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_slab_is_the_librarys():
    from gym_narde import _lib

    assert SLAB == _lib.TD_SLAB


@pytest.fixture(scope="module")
def pool():
    """The golden states, and among them the one-ply-to-win ones: the mover
    has borne off 14 and both dice bear the last checker off.  win[(colour,
    reward)] = their indices."""
    board, off, ft, player, dice = (np.asarray(a) for a in golden_states())
    mine = np.where(player[:, None] == 1, board, -np.roll(board, 12, axis=1))  # the mover's own counts, its points
    own = np.clip(mine, 0, None)
    m_off = np.where(player == 1, off[:, 0], off[:, 1])
    o_off = np.where(player == 1, off[:, 1], off[:, 0])
    last = own.argmax(1)
    sure = (m_off == 14) & (own.sum(1) == 1) & (last <= 5) & (dice.min(1) >= last + 1)
    win = {(c, r): np.nonzero(sure & (player == c) & ((o_off == 0) == (r == 2)))[0] for c in (1, -1) for r in (1, 2)}
    assert all(len(v) >= 4 for v in win.values()), {k: len(v) for k, v in win.items()}
    plain = np.nonzero(m_off < 12)[0]
    return dict(board=board, off=off, ft=ft, player=player, dice=dice, win=win, plain=plain)


def batch(pool, B):
    """B states: (B >= 8) envs 0..3 win -- white 2 points, black 1, white 1,
    black 2 --, env 4 has to pass (dice 0), env 5 truncates, the last env
    wins too; the rest are ordinary plies."""
    idx = pool["plain"][(np.arange(B) * 37) % len(pool["plain"])]
    plan = {}
    if B >= 8:
        for e, key in ((0, (1, 2)), (1, (-1, 1)), (2, (1, 1)), (3, (-1, 2)), (B - 1, (-1, 1))):
            idx[e] = pool["win"][key][1 if e == B - 1 else 0]
            plan[e] = key
    st = {k: np.ascontiguousarray(pool[k][idx]) for k in ("board", "off", "ft", "player", "dice")}
    st["elapsed"] = np.full(B, 3, np.int16)
    if B >= 8:
        st["dice"][4] = 0
        st["elapsed"][5] = MAX_STEPS - 1
    return st, plan


class Raw:
    """One net's weights and B trace rows in padded device arrays, the
    padding full of SENT: ld_w1t = hidden + 4, ld_w1 = 198 + 2, ld_trace =
    P rounded up + 8."""

    def __init__(self, cpu, dev, B, seed=0):
        from gym_narde import _lib
        from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

        H = cpu.hidden
        self.H, self.B, self.P = H, B, T.row_floats(H)
        self.ld, self.ld_w1, self.ldt = H + 4, 200, (self.P + 3) // 4 * 4 + 8
        f = dict(dtype=torch.float32, device=dev)
        self.w1t = torch.full((198, self.ld), SENT, **f)
        self.w1t[:, :H] = cpu.l1.weight.detach().t().to(dev)
        self.w1 = torch.full((H, self.ld_w1), SENT, **f)
        self.w1[:, :198] = cpu.l1.weight.detach().to(dev)
        self.b1 = cpu.l1.bias.detach().clone().to(dev)
        self.w2 = cpu.l2.weight.detach().reshape(-1).clone().to(dev)
        self.b2 = cpu.l2.bias.detach().clone().to(dev)
        g = torch.Generator().manual_seed(seed)
        self.trace = torch.full((B, self.ldt), SENT, **f)
        self.trace[:, :self.P] = (torch.randn((B, self.P), generator=g) * 0.1).to(dev)
        self.v = torch.full((B,), SENT, **f)
        self.black = torch.full((B,), 9, dtype=torch.uint8, device=dev)
        self.delta = torch.full((B,), SENT, **f)
        self.scratch = torch.empty(_lib.td_scratch_floats(B, H), **f)
        self.mlp = _lib.ValueMlpTrain(self.w1t.data_ptr(), self.ld, self.b1.data_ptr(), self.w2.data_ptr(),
                                      self.b2.data_ptr(), H, HIDDEN_ACTS[cpu.hidden_act], OUT_ACTS[cpu.out_act],
                                      self.w1.data_ptr(), self.ld_w1)

    def trace_call(self, env, decay):
        from gym_narde._lib import ptr

        env.handle.call("narde_value_td_trace", ctypes.byref(self.mlp), decay, ptr(self.trace), self.ldt, ptr(self.v),
                        ptr(self.black), env._s())

    def apply_call(self, env, reward, term, trunc, alpha, gamma):
        from gym_narde._lib import ptr

        env.handle.call("narde_value_td_apply", ctypes.byref(self.mlp), ptr(self.trace), self.ldt, ptr(self.v),
                        ptr(self.black), ptr(reward), ptr(term), ptr(trunc), alpha, gamma, 1, ptr(self.scratch),
                        self.scratch.numel(), ptr(self.delta), env._s())

    def params(self, dtype):
        """(W1, b1, w2, b2) on the CPU as dtype, from the device arrays."""
        c = lambda x: x.detach().cpu().to(dtype)  # noqa: E731
        return c(self.w1t[:, :self.H]).t().contiguous(), c(self.b1), c(self.w2), c(self.b2).reshape(())

    def theta(self):
        return T.theta_row(self.params(torch.float32)).numpy()

    def padding_untouched(self):
        assert (self.w1t[:, self.H:] == SENT).all() and (self.w1[:, 198:] == SENT).all()
        assert (self.trace[:, self.P:] == SENT).all()

    def mirror_is_exact(self):
        assert torch.equal(self.w1[:, :198].view(torch.int32), self.w1t[:, :self.H].t().contiguous().view(torch.int32))


def feat_of(st):
    return torch.from_numpy(O.tesauro198(np_(st["board"]) if torch.is_tensor(st["board"]) else st["board"],
                                         np_(st["off"]) if torch.is_tensor(st["off"]) else st["off"],
                                         np_(st["player"]) if torch.is_tensor(st["player"]) else st["player"]))


def reference(params32, params64, acts, x, x2, trace0, decay, reward, black, term, trunc, alpha, gamma):
    """{name: (fp32, fp64)} of one trace + apply: v, trace (after the trace
    pass), delta, theta (after the update), by td_ref's formulas."""
    out = {}
    res = []
    for p, dt in ((params32, torch.float32), (params64, torch.float64)):
        v, g = T.value_and_grad(p, x.to(dt), *acts)
        v2, _ = T.value_and_grad(p, x2.to(dt), *acts)
        tr = g if decay == 0 else torch.tensor(decay, dtype=dt) * trace0.to(dt) + g
        delta = T.td_targets(v, v2, reward, black, term, trunc, torch.tensor(gamma, dtype=dt))
        theta = T.theta_row(p) + torch.tensor(alpha, dtype=dt) * (delta[:, None] * tr).sum(0)
        res.append(dict(v=v, trace=tr, delta=delta, theta=theta))
    for k in res[0]:
        out[k] = (res[0][k].numpy(), res[1][k].numpy())
    return out


def close(what, got, pair):
    b = T.Bound(what)
    b.add(np_(got) if torch.is_tensor(got) else got, *pair)
    return b.check()


# every B of {1, S - 1, S, S + 1, 2 S + 1}, every H of {1, 16, 17, 65, 80, 128}, every activation pair
CASES = [(1, 80, "sigmoid", "sigmoid"), (SLAB - 1, 1, "relu", "none"), (SLAB, 16, "tanh", "tanh"),
         (SLAB + 1, 17, "sigmoid", "none"), (2 * SLAB + 1, 65, "relu", "tanh"), (SLAB + 1, 128, "tanh", "none"),
         (SLAB, 80, "relu", "sigmoid"), (2 * SLAB + 1, 16, "sigmoid", "tanh"), (SLAB - 1, 128, "tanh", "sigmoid")]


@pytest.mark.parametrize("B,H,hact,oact", CASES, ids=lambda x: str(x))
def test_trace_step_apply_against_float64(pool, B, H, hact, oact):
    from gym_narde.vector import VecNardeEnv

    st, plan = batch(pool, B)
    env = VecNardeEnv(B, device="cuda:0", seed=5, autoreset=True, max_episode_steps=MAX_STEPS)
    env.set_state(st["board"], st["off"], st["ft"], st["player"], st["elapsed"])
    cpu = make_net(H, hact, oact, seed=H)
    raw = Raw(cpu, env.device, B)
    decay, alpha, gamma = 0.7, 0.05, 0.9
    p32, p64 = raw.params(torch.float32), raw.params(torch.float64)
    trace0 = raw.trace[:, :raw.P].cpu()
    raw.trace_call(env, decay)
    trace1 = raw.trace.clone()
    _, reward, term, trunc, _ = env.step(None, st["dice"])
    post = env.get_state()
    raw.apply_call(env, reward, term, trunc, alpha, gamma)
    torch.cuda.synchronize()
    reward, term, trunc = reward.cpu(), term.cpu(), trunc.cpu()
    # the batch holds what it was built to hold
    for e, (colour, r) in plan.items():
        assert term[e] == 1 and reward[e] == r and st["player"][e] == colour, e
    if B >= 8:
        assert trunc[5] == 1 and term[5] == 0 and term[4] == 0 and trunc[4] == 0
        assert np.array_equal(np_(post["board"])[4], st["board"][4]) and np_(post["player"])[4] == -st["player"][4]
        assert ((term == 0) & (trunc == 0)).sum() >= B - 8
    black = torch.from_numpy((st["player"] == -1).astype(np.uint8))
    assert torch.equal(raw.black.cpu(), black)
    want = reference(p32, p64, (hact, oact), feat_of(st), feat_of(post), trace0, decay, reward, black, term, trunc,
                     alpha, gamma)
    what = f"B={B} H={H} {hact}/{oact}"
    close(f"v {what}", raw.v, want["v"])
    close(f"trace {what}", trace1[:, :raw.P], want["trace"])
    close(f"delta {what}", raw.delta, want["delta"])
    close(f"theta {what}", raw.theta(), want["theta"])
    d = np_(raw.delta)
    assert (d[np_(trunc).astype(bool) & ~np_(term).astype(bool)] == 0).all()
    # the update moved the weights far beyond the tolerance: a wrong sum would show
    assert np.abs(want["theta"][1] - T.theta_row(p64).numpy()).max() > 1e3 * np.spacing(np.float32(np.abs(want["theta"][1]).max()))
    # done envs' rows are zero, the others' are what the trace pass left, bit for bit
    done = (term | trunc).bool()
    after = raw.trace[:, :raw.P].cpu()
    assert (after[done] == 0).all()
    assert torch.equal(after[~done].view(torch.int32), trace1[:, :raw.P].cpu()[~done].view(torch.int32))
    raw.padding_untouched()
    raw.mirror_is_exact()
    env.close()


def test_decay_zero_overwrites_without_reading(pool):
    from gym_narde.vector import VecNardeEnv

    B = SLAB + 1
    st, _ = batch(pool, B)
    env = VecNardeEnv(B, device="cuda:0", seed=5, autoreset=True)
    env.set_state(st["board"], st["off"], st["ft"], st["player"], st["elapsed"])
    cpu = make_net(17, "tanh", "tanh", seed=4)
    raw = Raw(cpu, env.device, B)
    raw.trace[:, :raw.P] = float("nan")
    raw.trace_call(env, 0.0)
    torch.cuda.synchronize()
    x = feat_of(st)
    pair = [T.value_and_grad(raw.params(dt), x.to(dt), "tanh", "tanh")[1].numpy() for dt in (torch.float32, torch.float64)]
    close("trace decay 0", raw.trace[:, :raw.P], pair)
    raw.padding_untouched()
    env.close()


def snapshot(learner):
    net = learner.net
    return (T.params_of(net, torch.float32, "cpu"), T.params_of(net, torch.float64, "cpu"),
            learner.trace[:, :learner.row_floats].cpu())


@pytest.mark.parametrize("lam", [0.0, 0.7])
@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_ten_learner_steps_teacher_forced(rules, lam):
    """Each ply's reference starts from the GPU's own weights and traces of
    the ply before, so rounding does not compound."""
    from gym_narde.td import TDLambdaLearner
    from gym_narde.vector import VecNardeEnv

    B, alpha, gamma = 65, 0.02, 0.95
    env = VecNardeEnv(B, device="cuda:0", seed=11, rules=rules, max_episode_steps=64)
    env.selfplay(55)  # the middle game; the envs truncate at seven different plies of the ten
    st = env.get_state()
    stagger = (torch.arange(B, device=env.device) % 7).to(torch.int16)
    env.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"] + stagger)
    acts = ("sigmoid", "tanh")
    net = copy.deepcopy(make_net(80, *acts, seed=9)).to(env.device)
    learner = TDLambdaLearner(env, net, alpha=alpha, lam=lam, gamma=gamma, epsilon=0.1, seed=3)
    assert learner.memory_bytes() >= B * learner.ld_trace * 4
    worst = 0.0
    ended = 0
    for ply in range(10):
        p32, p64, trace0 = snapshot(learner)
        pre = env.get_state()
        out = learner.step()
        reward, term, trunc, delta = out[1].cpu(), out[2].cpu(), out[3].cpu(), out[-1]
        post = env.get_state()
        torch.cuda.synchronize()
        black = (pre["player"] == -1).to(torch.uint8).cpu()
        want = reference(p32, p64, acts, feat_of(pre), feat_of(post), trace0, gamma * lam, reward, black, term, trunc,
                         alpha, gamma)
        what = f"{rules} lam={lam} ply {ply}"
        worst = max(worst, close(f"v {what}", learner.v, want["v"]), close(f"delta {what}", delta, want["delta"]),
                    close(f"theta {what}", T.theta_row(T.params_of(net, torch.float32, "cpu")).numpy(), want["theta"]))
        done = (term | trunc).bool()
        ended += int(done.sum())
        tr = learner.trace[:, :learner.row_floats].cpu()
        assert (tr[done] == 0).all()
        # lam = 0: want["trace"] is that ply's gradient alone
        worst = max(worst, close(f"trace {what}", tr[~done], tuple(a[np_(~done)] for a in want["trace"])))
        named = learner.traces()
        assert named["l1.weight"].shape == (B,) + tuple(net.l1.weight.shape)
        assert named["l2.weight"].shape == (B,) + tuple(net.l2.weight.shape)
        assert torch.equal(named["l1.weight"][:, 3, 7].cpu(), tr[:, 7 * 80 + 3]) and named["l1.bias"].shape == (B, 80)
        assert torch.equal(net._w1t.view(torch.int32), net.l1.weight.t().contiguous().view(torch.int32))
    assert ended > 0
    print(f"{rules} lam={lam}: worst ratio {worst:.2f} E")
    env.close()


def test_learner_refuses_what_it_cannot_run(monkeypatch):
    from gym_narde.td import TDLambdaLearner
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device="cuda:0", seed=1)
    net = make_net(16, "sigmoid", "tanh", seed=1)
    with pytest.raises(ValueError, match="is on"):
        TDLambdaLearner(env, net, alpha=0.1, lam=0.5)  # the net is on the CPU
    net = net.to(env.device)
    with pytest.raises(TypeError):
        TDLambdaLearner(env, torch.nn.Linear(198, 1).to(env.device), alpha=0.1, lam=0.5)
    fixed = VecNardeEnv(8, device="cuda:0", seed=1, autoreset=False)
    with pytest.raises(ValueError, match="autoreset"):
        TDLambdaLearner(fixed, net, alpha=0.1, lam=0.5)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (1000, 1 << 30))
    with pytest.raises(ValueError, match="free"):
        TDLambdaLearner(env, net, alpha=0.1, lam=0.5)
    monkeypatch.undo()
    learner = TDLambdaLearner(env, net, alpha=0.1, lam=0.5)
    assert learner.memory_bytes() == 4 * (8 * learner.ld_trace + 8 + 8 + learner.scratch.numel()) + 8
    fixed.close()
    env.close()


def run_plies(seed, plies=10):
    from gym_narde.td import TDLambdaLearner
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(2 * SLAB + 1, device="cuda:0", seed=seed, max_episode_steps=40)
    env.selfplay(30)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=2)).to(env.device)
    learner = TDLambdaLearner(env, net, alpha=0.01, lam=0.7, epsilon=0.1, seed=seed)
    for _ in range(plies):
        learner.step()
    torch.cuda.synchronize()
    out = [p.detach().cpu().clone() for p in net.parameters()] + [net._w1t.cpu().clone(), learner.trace.cpu().clone()]
    env.close()
    return out


def test_same_seed_same_bits():
    a, b = run_plies(21), run_plies(21)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[0], make_net(80, "sigmoid", "tanh", seed=2).l1.weight.detach())  # it did learn


def test_scored_calls_see_the_update_without_pack():
    from gym_narde.td import TDLambdaLearner
    from gym_narde.vector import VecNardeEnv
    from test_gpu_value import check_values, expected

    env = VecNardeEnv(257, device="cuda:0", seed=8)
    env.selfplay(40)
    net = copy.deepcopy(make_net(80, "sigmoid", "sigmoid", seed=1)).to(env.device)
    before = net.l1.weight.detach().clone()
    learner = TDLambdaLearner(env, net, alpha=0.05, lam=0.7)

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
    check_values(values, want, E, term, "after three updates")
    # and the dense forward is the same net
    x = env.tesauro198()
    v64 = T.value_and_grad(T.params_of(net, torch.float64, "cpu"), x.cpu().double(), "sigmoid", "sigmoid")[0]
    v32 = T.value_and_grad(T.params_of(net, torch.float32, "cpu"), x.cpu(), "sigmoid", "sigmoid")[0]
    with torch.no_grad():
        close("net(feat)", net(x), (v32.numpy(), v64.numpy()))
    env.close()


def test_graph_replay_equals_eager(pool):
    """trace + apply captured on one stream, replayed once: the eager bits."""
    from gym_narde.vector import VecNardeEnv

    B = 2 * SLAB + 1
    st, _ = batch(pool, B)
    env = VecNardeEnv(B, device="cuda:0", seed=5, autoreset=True)
    env.set_state(st["board"], st["off"], st["ft"], st["player"], st["elapsed"])
    dev = env.device
    cpu = make_net(80, "sigmoid", "tanh", seed=6)
    raw = Raw(cpu, dev, B)
    g = torch.Generator().manual_seed(1)
    term = (torch.rand(B, generator=g) < 0.2).to(torch.uint8).to(dev)
    trunc = (torch.rand(B, generator=g) < 0.2).to(torch.uint8).to(dev)
    reward = (term.cpu().int() * torch.randint(1, 3, (B,), generator=g, dtype=torch.int32)).to(dev)
    arrays = (raw.w1t, raw.w1, raw.b1, raw.w2, raw.b2, raw.trace, raw.v, raw.black, raw.delta)
    start = [a.clone() for a in arrays]

    def both():
        raw.trace_call(env, 0.7)
        raw.apply_call(env, reward, term, trunc, 0.05, 0.9)

    both()
    torch.cuda.synchronize()
    eager = [a.clone() for a in arrays]
    for a, s in zip(arrays, start):
        a.copy_(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, s in zip(arrays, start):  # capture ran nothing
        assert torch.equal(a, s)
    graph.replay()
    torch.cuda.synchronize()
    for a, want in zip(arrays, eager):
        assert torch.equal(a.view(torch.uint8), want.view(torch.uint8))
    assert not torch.equal(raw.b1, start[2])
    env.close()


def test_the_learner_learns_a_fixed_regression(pool):
    """64 one-ply-to-win positions, reset every iteration; lam 0, linear
    output: gradient descent of v(s) towards the outcomes, so the mean TD
    error shrinks."""
    from gym_narde.td import TDLambdaLearner
    from gym_narde.vector import VecNardeEnv

    B = 64
    keys = sorted(pool["win"])
    idx = np.concatenate([pool["win"][k] for k in keys])
    idx = idx[(np.arange(B) * 5) % len(idx)]
    st = {k: np.ascontiguousarray(pool[k][idx]) for k in ("board", "off", "ft", "player", "dice")}
    env = VecNardeEnv(B, device="cuda:0", seed=1)
    net = copy.deepcopy(make_net(40, "sigmoid", "none", seed=3, scale=1.0)).to(env.device)
    learner = TDLambdaLearner(env, net, alpha=2e-4, lam=0.0)
    errs = []
    for _ in range(31):
        env.set_state(st["board"], st["off"], st["ft"], st["player"])
        learner.trace_pass()
        _, reward, term, trunc, _ = env.step(None, st["dice"])
        learner.apply_pass(reward, term, trunc)
        assert bool(term.all())
        errs.append(float(learner.delta.abs().mean()))
    print(f"mean |delta|: first {errs[0]:.4f}, after 30 updates {errs[-1]:.4f}")
    assert errs[-1] < errs[0]
    env.close()


def test_the_training_example_writes_loadable_weights(tmp_path):
    from gym_narde.value_net import ValueMLP

    out = tmp_path / "agent.pt"
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "train_value_agent.py"),
           "--envs", "64", "--plies", "20", "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "saved" in res.stdout
    sd = torch.load(out, map_location="cpu")
    net = ValueMLP(80, "sigmoid", "tanh")
    net.load_state_dict(sd)
    assert all(torch.isfinite(p).all() for p in net.parameters())
