"""The supervised fit on the GPU: narde_value_fit and
narde_playout_targets (kernels_value_fit.h), VecNardeEnv.playout_targets,
gym_narde.td.ValueFitter and PlayoutTargetLearner.

Reference for the fit: narde.h's semantics in torch float64
(test_value_fit_cpu.reference) on O.tesauro198 rows of the records.
Tolerance: 8 x E, E = max |the same formulas in float32 - float64| per
compared array, floored at one float32 ulp of its largest magnitude -- td_ref's
rule, never a figure of the code under test.  The loss, the targets, and the
all-terminated window against narde_value_td_window are compared exactly.
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
from test_value_cpu import make_net
from test_value_fit_cpu import loss_restated, numpy_targets, reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import np_  # noqa: E402
from test_gpu_td_window import DEV, SENT, RawNet, middle_game, unpack_record, window_call  # noqa: E402

ALPHA = 0.01
ACTS = [(h, o) for h in ("sigmoid", "tanh", "relu") for o in ("none", "sigmoid", "tanh")]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def recorded():
    """Per rule set 390 records and their feature rows: two 3-ply records
    rollouts at B = 65, epsilon 0.2 (one launch gives 195, n = 300 needs more),
    with seeded random targets in [-2, 2]."""
    out = {}
    for rules in ("ref2", "full4"):
        env = middle_game(rules, 65)
        net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=5)).to(env.device)
        make = env.turn_value_rollout_buffers if env.full else env.value_rollout_buffers
        roll = env.turn_value_rollout if env.full else env.value_rollout
        parts = []
        for launch in range(2):
            bufs = roll(3, net, epsilon=0.2, tag=3 * launch, seed=4, bufs=make(3, records=True))
            parts.append(bufs["records"].reshape(-1, 8).clone())
        records = torch.cat(parts).contiguous()
        torch.cuda.synchronize()
        board, off, player = unpack_record(np_(records))
        assert (player == 1).any() and (player == -1).any()
        target = (np.random.default_rng(17).random(len(player)) * 4 - 2).astype(np.float32)
        out[rules] = (env, records, O.tesauro198(board, off, player), target)
    yield out
    for env, *_ in out.values():
        env.close()


def fit_call(env, mlp, records, target, weight, alpha, H, want_v=True, want_loss=True):
    """narde_value_fit with sentinels behind the scratch: (v, loss) on the host."""
    from gym_narde import _lib

    n = int(records.shape[0])
    need = _lib.value_fit_scratch_floats(n, H)
    scratch = torch.full((need + 4,), SENT, dtype=torch.float32, device=env.device)
    v = torch.full((n,), SENT, dtype=torch.float32, device=env.device) if want_v else None
    loss = torch.full((2,), SENT, dtype=torch.float64, device=env.device) if want_loss else None
    dev = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float32).to(env.device)  # noqa: E731
    tg, wt = dev(target), dev(weight)
    _lib.check(env.handle.lib.narde_value_fit(env.device.index, ctypes.byref(mlp), n, _lib.ptr(records), _lib.ptr(tg),
                                              _lib.ptr(wt), alpha, _lib.ptr(scratch), need, _lib.ptr(v), _lib.ptr(loss),
                                              env._s()), "narde_value_fit")
    torch.cuda.synchronize()
    assert (scratch[need:] == SENT).all()
    return (np_(v) if want_v else None), (np_(loss) if want_loss else None)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


FIT_CASES = [(n, H, ACTS[(i + 2 * j) % 9], ("ref2", "full4")[(i + j) % 2], 4 * ((i + j) % 2))
             for i, n in enumerate((1, 127, 129, 300)) for j, H in enumerate((1, 17, 80, 128))]
FIT_CASES += [(129, 17, acts, ("ref2", "full4")[i % 2], 0) for i, acts in enumerate(ACTS)]


@pytest.mark.parametrize("n,H,acts,rules,pad", FIT_CASES, ids=lambda x: "-".join(x) if isinstance(x, tuple) else str(x))
def test_fit_against_float64(recorded, n, H, acts, rules, pad):
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
    worst, base = 0.0, None
    for name, t_in, w_in in (("NULL", tg, None), ("ones", tg, np.ones(n, np.float32)), ("mixed", t_nan, mixed)):
        raw = RawNet(cpu, env.device, pad)
        p32, p64 = raw.params(torch.float32), raw.params(torch.float64)
        v, loss = fit_call(env, raw.mlp, rec, t_in, w_in, ALPHA, H)
        r32, r64 = (reference(p, ft, t_in, w_in, ALPHA, *acts) for p in (p32, p64))
        for key, g, a, b in zip(("v", "theta"), (v, raw.theta()), r32, r64):
            bd = T.Bound(f"{key} {what} weights={name}")
            bd.add(g, a.numpy(), b.numpy())
            worst = max(worst, bd.check())
        moved = float((r64[1] - T.theta_row(p64)).abs().max())
        assert moved > 10 * T.TOL_FACTOR * float(np.spacing(np.float32(r64[1].abs().max())))  # a lost update would show
        assert np.array_equal(loss, loss_restated(v, t_in, w_in)), (what, name)
        raw.checks()  # the mirror transposed bit for bit, the padding of both untouched
        if name == "NULL":
            base = (v, loss, raw.theta())
        else:
            assert np.array_equal(bits(v), bits(base[0]))
        if name == "ones":
            assert np.array_equal(bits(raw.theta()), bits(base[2])) and np.array_equal(loss, base[1])
    print(f"{what}: worst ratio {worst:.2f} E")
    # what moves no weight bit: every weight zero (targets NaN), alpha = 0, target = the call's own v
    raw = RawNet(cpu, env.device, pad)
    theta0 = raw.theta()
    _, loss = fit_call(env, raw.mlp, rec, np.full(n, np.nan, np.float32), np.zeros(n, np.float32), ALPHA, H)
    assert np.array_equal(bits(raw.theta()), bits(theta0)) and np.array_equal(loss, [0.0, 0.0])
    v, loss = fit_call(env, raw.mlp, rec, tg, None, 0.0, H)
    assert np.array_equal(bits(raw.theta()), bits(theta0)) and np.array_equal(loss, loss_restated(v, tg, None))
    assert np.array_equal(bits(v), bits(base[0])) and loss[1] == n
    v2, loss = fit_call(env, raw.mlp, rec, v, None, 0.05, H)
    assert np.array_equal(bits(raw.theta()), bits(theta0)) and loss[0] == 0.0 and np.array_equal(bits(v2), bits(v))
    fit_call(env, raw.mlp, rec, tg, None, 0.0, H, want_v=False, want_loss=False)  # both optional outputs NULL
    assert np.array_equal(bits(raw.theta()), bits(theta0))
    raw.checks()


@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_all_terminated_window_gives_the_window_updates_bits(rules):
    """The yardstick is narde_value_td_window: every ply terminated, gamma = 1,
    so G_k = outcome - v_k, and the fit of the same K B records onto the
    outcomes must move every weight to the same bits."""
    B, K, H = 65, 3, 80
    env = middle_game(rules, B)
    cpu = make_net(H, "sigmoid", "tanh", seed=21)
    net = copy.deepcopy(cpu).to(env.device)
    make = env.turn_value_rollout_buffers if env.full else env.value_rollout_buffers
    bufs = (env.turn_value_rollout if env.full else env.value_rollout)(K, net, epsilon=0.2, tag=0, seed=4,
                                                                       bufs=make(K, records=True))
    torch.cuda.synchronize()
    records = bufs["records"].reshape(K * B, 8).contiguous()
    _, _, player = unpack_record(np_(records))
    black = player == -1
    reward = (1 + (np.arange(K * B) // 2) % 2).astype(np.int32)
    assert {(int(r), bool(b)) for r, b in zip(reward, black)} == {(1, False), (1, True), (2, False), (2, True)}
    forced = dict(records=bufs["records"], reward=torch.from_numpy(reward).reshape(K, B).to(env.device),
                  terminated=torch.ones((K, B), dtype=torch.uint8, device=env.device),
                  truncated=torch.zeros((K, B), dtype=torch.uint8, device=env.device))
    win, fit = RawNet(cpu, env.device, 4), RawNet(cpu, env.device, 4)
    v_win, _ = window_call(env, win.mlp, K, forced, 0.05, 0.7, 1.0, H)
    v_fit, _ = fit_call(env, fit.mlp, records, np.where(black, -reward, reward).astype(np.float32), None, 0.05, H)
    assert np.array_equal(bits(v_fit), bits(np_(v_win)[:K].reshape(-1)))
    assert np.array_equal(bits(fit.theta()), bits(win.theta()))
    assert not np.array_equal(bits(fit.theta()), bits(RawNet(cpu, env.device, 4).theta()))
    fit.checks()
    env.close()


# ------------------------------------------------------------------ playout_targets()
@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_targets_are_the_picks_scores_on_the_players_candidates(rules):
    """PlayoutPlayer's chain by hand -- recorded rows, top-K roots, playouts --,
    then pick_playout()'s score against playout_targets() slot by slot."""
    from gym_narde.vector import VecNardeEnv

    B, k, trials = 100, 3, 4
    env = VecNardeEnv(B, device=DEV, seed=31, rules=rules)
    env.selfplay(60)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=5)).to(env.device)
    aft, values, records = (env.recorded_turn_afterstates if env.full else env.recorded_afterstates)(net, env.dice())
    sel, roots = env.top_rows(aft, values, k, records)
    res = env.playout(roots, trials, net, max_plies=6, seed=77, common_dice=True, leaf=True)
    flat = np_(sel).reshape(-1)
    terminal = (flat >= 0) & (np_(aft.reward)[np.maximum(flat, 0)] != 0)
    fin = np_(res.finished)
    for leaf in (False, True):
        _, _, score = env.pick_playout(aft, values, sel, res, leaf=leaf)
        target, weight = env.playout_targets(res, roots=roots, leaf=leaf)
        plain_t, plain_w = env.playout_targets((res.sums, trials, res.leaf), leaf=leaf)
        torch.cuda.synchronize()
        sc, tg, wt = np_(score).reshape(-1), np_(target), np_(weight)
        live = (flat >= 0) & ~terminal & ((fin > 0) | leaf)
        assert (live.sum() > B or not leaf) and np.array_equal(wt[live], np.ones(live.sum(), np.float32))
        assert np.array_equal(bits(tg[live]), bits(sc[live]))
        dead = (flat < 0) | terminal
        assert (wt[dead] == 0).all() and (tg[dead] == 0).all()
        rest = ~live & ~dead  # no trial finished and no leaves
        assert (wt[rest] == 0).all() and (tg[rest] == 0).all() and (leaf or rest.any())
        want_t, want_w = numpy_targets(np_(res.sums), np_(res.leaf) if leaf else None, trials, np_(roots).view(np.uint32))
        assert np.array_equal(bits(tg), bits(want_t)) and np.array_equal(bits(wt), bits(want_w))
        # without roots a terminal row's record is not recognised: the sums' own numbers
        want_t, want_w = numpy_targets(np_(res.sums), np_(res.leaf) if leaf else None, trials, None)
        assert np.array_equal(bits(np_(plain_t)), bits(want_t)) and np.array_equal(bits(np_(plain_w)), bits(want_w))
    out = (torch.zeros_like(target), torch.zeros_like(weight))
    assert env.playout_targets(res, roots=roots, leaf=True, out=out)[0] is out[0]
    torch.cuda.synchronize()
    assert torch.equal(out[0], target) and torch.equal(out[1], weight)
    with pytest.raises(ValueError, match="leaf"):
        env.playout_targets((res.sums, trials), leaf=True)
    env.close()


@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_targets_of_finished_playouts_are_the_mean_outcomes(rules):
    from gym_narde.vector import VecNardeEnv
    from test_value_playout_cpu import late_races
    from test_value_rollout_cpu import endgames

    env = VecNardeEnv(1, device=DEV, seed=2, rules=rules)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=5)).to(env.device)
    state = tuple(np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(late_races(), endgames()))
    roots = env.state_records(*state)
    trials = 4
    res = env.playout(roots, trials, net, max_plies=40, seed=5, leaf=True)
    for leaf in (False, True):
        target, weight = env.playout_targets(res, roots=roots, leaf=leaf)
        torch.cuda.synchronize()
        assert (np_(res.finished) == trials).all()
        want_t, want_w = numpy_targets(np_(res.sums), np_(res.leaf) if leaf else None, trials, np_(roots).view(np.uint32))
        assert np.array_equal(bits(np_(target)), bits(want_t)) and np.array_equal(bits(np_(weight)), bits(want_w))
        assert (np_(weight) == 1).all() and np.array_equal(np_(target), (np_(res.points) / 4.0).astype(np.float32))
    env.close()


# ------------------------------------------------------------------ PlayoutTargetLearner
def make_learner(rules, seed=3):
    from gym_narde.td import PlayoutTargetLearner

    env = middle_game(rules, 65, max_steps=48, seed=11)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=9)).to(env.device)
    return PlayoutTargetLearner(env, net, alpha=0.002, plies=3, trials=4, max_plies=6, leaf=True, epsilon=0.1, seed=seed)


def learner_bits(learner):
    out = [p.detach().clone() for p in learner.net.parameters()] + [learner.net._w1t.clone()]
    out += [learner.roots.clone(), learner.target.clone(), learner.weight.clone(), learner.fitter.loss.clone()]
    out += [v.clone() for v in learner.bufs.values()] + list(learner.env.get_state().values())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_four_learner_steps(rules):
    """Four steps run twice give the same bits, and with the fourth captured as
    one graph and replayed once; the fourth, teacher-forced against float64 on
    the learner's own records and targets, is within 8 E; the scored calls see
    the weights with no pack(); the env's statistics move only by play()."""
    from test_gpu_value import check_values, expected

    runs = []
    for mode in ("checked", "eager", "graph"):
        learner = make_learner(rules)
        env, net = learner.env, learner.net
        N = learner.roots.shape[0]
        assert N == 3 * 65
        for step in range(3):
            if mode == "checked" and step == 0:
                s0 = env.stats().clone()
                learner.play()
                s1 = env.stats().clone()
                learner.targets()
                learner.update()
                s2 = env.stats().clone()
                assert torch.equal(s1, s2) and not torch.equal(s0, s1)
            else:
                learner.step()
        torch.cuda.synchronize()
        assert learner.windows == 3 and int(learner._tag) == 9
        if mode == "checked":
            def no_pack():
                raise AssertionError("pack() called")

            net.pack = no_pack
            p32, p64 = T.params_of(net, torch.float32, "cpu"), T.params_of(net, torch.float64, "cpu")
            loss, target, weight = learner.step()
            torch.cuda.synchronize()
            assert loss.shape == (2,) and loss.dtype == torch.float64 and target.shape == weight.shape == (N,)
            assert torch.equal(learner.roots.view(3, 65, 8), learner.bufs["records"])
            board, off, player = unpack_record(np_(learner.roots))
            feat = O.tesauro198(board, off, player)
            tg, wt = np_(target), np_(weight)
            assert (wt == 1).all() and not np.isnan(tg).any() and (np.abs(tg) <= 2).all()  # leaves: every root counts
            r32, r64 = (reference(p, feat, tg, wt, learner.alpha, net.hidden_act, net.out_act) for p in (p32, p64))
            got = (np_(learner.values()), T.theta_row(T.params_of(net, torch.float32, "cpu")).numpy())
            for key, g, a, b in zip(("v", "theta"), got, r32, r64):
                bd = T.Bound(f"{key} {rules} step 4")
                bd.add(g, a.numpy(), b.numpy())
                print(f"{rules} step 4 {key}: {bd.check():.2f} E")
            assert np.array_equal(np_(loss), loss_restated(got[0], tg, wt))
            assert torch.equal(net._w1t.view(torch.int32), net.l1.weight.t().contiguous().view(torch.int32))
            assert learner.memory_bytes() >= 4 * learner.fitter.scratch.numel() + 32 * N * 2
            if rules == "ref2":
                plain = env.afterstates()
                aft, values = env.scored_afterstates(net, perspective="white")
                want, E, term = expected(copy.deepcopy(net).cpu(), plain.feat, plain.reward, "white")
                check_values(values, want, E, term, "after four fits")
        elif mode == "eager":
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
        env.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert not torch.equal(runs[0][0].cpu(), make_net(80, "sigmoid", "tanh", seed=9).l1.weight.detach())  # it did learn


def test_fitter_and_learner_refuse_what_they_cannot_run():
    from gym_narde.td import PlayoutTargetLearner, ValueFitter
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device=DEV, seed=1)
    net = make_net(16, "sigmoid", "tanh", seed=1)
    with pytest.raises(ValueError, match="is on"):
        ValueFitter(env, net, 8)  # the net is on the CPU
    net = net.to(env.device)
    with pytest.raises(TypeError):
        ValueFitter(env, torch.nn.Linear(198, 1).to(env.device), 8)
    fixed = VecNardeEnv(8, device=DEV, seed=1, autoreset=False)
    with pytest.raises(ValueError, match="autoreset"):
        PlayoutTargetLearner(fixed, net, alpha=0.1, plies=4, trials=2)
    with pytest.raises(ValueError, match="every"):
        PlayoutTargetLearner(env, net, alpha=0.1, plies=4, trials=2, every=0)
    learner = PlayoutTargetLearner(env, net, alpha=0.1, plies=5, trials=2, every=2)
    assert learner.roots.shape == (3 * 8, 8)  # plies 0, 2, 4
    fit = ValueFitter(env, net, 8)
    st = env.get_state()
    records = env.state_records(st["board"], st["off"], st["first_turn"], st["player"])
    with pytest.raises(ValueError, match="samples"):
        fit.step(torch.cat([records, records]), torch.zeros(16), alpha=0.1)
    with pytest.raises(ValueError, match="records"):
        fit.step(records[:, :4].contiguous(), torch.zeros(8), alpha=0.1)
    fixed.close()
    env.close()


# ------------------------------------------------------------------ learning
def test_fits_lower_the_loss_on_known_outcomes():
    """64 fixed positions whose answer is known: the mover has borne off 14 and
    its last checker stands on its lowest point, so any roll ends the game --
    both colours, the loser with 0 .. 12 off (1 or 2 points).  Their playout
    targets are the winner's points, and 30 fits at alpha 2e-4 lower the mean
    squared error against them."""
    from gym_narde.td import ValueFitter
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
    torch.cuda.synchronize()
    tg = np_(target)
    assert (np_(res.finished) == trials).all() and (np_(weight) == 1).all()
    assert set(np.unique(np.abs(tg))) <= {1.0, 2.0} and (np.sign(tg) == player).all()
    fit = ValueFitter(env, net, B)
    first = fit.evaluate(roots, target, weight).clone()
    for _ in range(30):
        fit.step(roots, target, weight, alpha=2e-4)
    last = fit.evaluate(roots, target, weight).clone()
    torch.cuda.synchronize()
    a, b = float(first[0] / first[1]), float(last[0] / last[1])
    print(f"mean squared error: first {a:.4f}, after 30 fits {b:.4f}")
    assert b < a
    env.close()


def test_the_training_example_trains_on_playout_targets(tmp_path):
    from gym_narde.value_net import ValueMLP

    out = tmp_path / "agent.pt"
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "train_value_agent.py"),
           "--window", "4", "--playout-targets", "4", "--envs", "64", "--plies", "12", "--max-plies", "8", "--leaf",
           "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "saved" in res.stdout
    net = ValueMLP(80, "sigmoid", "tanh")
    net.load_state_dict(torch.load(out, map_location="cpu"))
    assert all(torch.isfinite(p).all() for p in net.parameters())
