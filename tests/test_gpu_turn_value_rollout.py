"""The FULL4 value rollout on the GPU (k_turn_value_rollout through
VecNardeEnv.turn_value_rollout, value_play.play_turn_match and the C call;
DESIGN.md section 20), replayed against calls that existed before it.

A second rules="full4" env with the same seed and ids has the same device
dice and opening rolls.  Per ply: env2.dice() is the recorded roll;
env2.turn_afterstates(feat) gives the rows, the CPU twins of the nets their
reference values in float64 (and E, from the float32 pass);
env2.scored_turn_afterstates() under each net, selected by the mover, and
env2.pick_turn(epsilon, tag + k, seed) give what the composed path plays;
env2.step(the recorded play) gives the reward and the flags.  The judgement of
a greedy ply is tests/test_turn_value_rollout_cpu.py's (teacher-forced: the
recorded play must be a row; the reference's arg-best where its gap exceeds
8 E, else within 8 E of it; at most 1 % exempt).  Explore plies and random
plies match the existing calls exactly.
"""
import copy
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT
from test_value_cpu import make_net
from test_value_rollout_cpu import M32, endgames, judge, mulhi
from turn_afterstates_ref import BIG_ROWS, big_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, ENV0, PICK_SEED, TAG = 20251020, 3, 91, 500
SAME = object()
H80 = (80, "sigmoid", "sigmoid", 1)
H1 = (1, "tanh", "none", 3)
H17 = (17, "tanh", "none", 6)
H128 = (128, "sigmoid", "sigmoid", 2)
KEYS = ("dice", "play", "value", "reward", "terminated", "truncated")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def np_(x):
    return x.detach().cpu().numpy()


def make_env(B, max_steps=1000, state=None, rules="full4"):
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(B, device="cuda:0", seed=SEED, env_id_offset=ENV0, max_episode_steps=max_steps, rules=rules)
    if state is not None:
        env.set_state(*(torch.as_tensor(a).to(env.device) for a in state))
    return env


def twins(spec, device):
    if spec is None:
        return None, None
    cpu = make_net(*spec)
    return copy.deepcopy(cpu).to(device), cpu


def snapshot(env):
    st = {k: np_(v) for k, v in env.get_state().items()}
    return st, np_(env.stats()), int(env.ply)


def assert_same_env(a, b):
    (sa, ta, pa), (sb, tb, pb) = snapshot(a), snapshot(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(ta, tb) and pa == pb


def assert_same_bufs(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(np_(a[k]).view(np.uint8), np_(b[k]).view(np.uint8)), f"{what} {k}"


def replay(env2, bufs, plies, gw, cw, gb, cb, eps=None, max_steps=1000):
    """Walk env2 through the recorded plies with the existing calls."""
    B = env2.num_envs
    J = dict(gap=[], is_best=[], short=[], verr=[], e32=0.0, mag=0.0, norow=0, explored=0, random=0, greedy=0,
             value_bits_equal=0, play_equals_pick=0, terminal_pick=0, resets=0, most_rows=0, greedy_above_64=0,
             above_256=0, explore_ordinal_64=0)
    out = {k: np_(v) for k, v in bufs.items() if v is not None}
    eps_q = None if eps is None else int(float(np.float32(eps)) * 4294967296.0)
    for k in range(plies):
        dice = env2.dice()
        assert np.array_equal(np_(dice), out["dice"][k]), f"ply {k}: dice"
        st = env2.get_state()
        player = np_(st["player"])
        rand_play = None
        if gw is None or gb is None:  # the random colour's plies: step() with no play, from the same state
            env3 = make_env(B, max_steps=max_steps)
            env3.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"])
            env3.ply = env2.ply
            rand_play = np_(env3.step()[4]["played"]).view(np.int8).reshape(B, 4, 2)
            env3.close()
        aft = env2.turn_afterstates(dice=dice, feat=True)
        offs, plays, reward = np_(aft.offsets), np_(aft.play), np_(aft.reward)
        feat = np_(aft.feat) if aft.cap else np.zeros((0, 198), np.float32)
        row_black = player[np_(aft.row_env)] == -1 if aft.cap else np.zeros(0, bool)
        v32 = np.zeros(aft.cap)
        v64 = np.zeros(aft.cap)
        vdev = torch.full((max(aft.cap, 1),), float("nan"), dtype=torch.float32, device=env2.device)
        scored = aft
        for black, g, c in ((False, gw, cw), (True, gb, cb)):
            sel = row_black == black
            if g is None or not aft.cap:
                continue
            scored, vals = env2.scored_turn_afterstates(g, dice=dice, cap=aft.cap)
            assert np.array_equal(np_(scored.play), plays)
            m = torch.from_numpy(sel).to(env2.device)
            vdev[:aft.cap] = torch.where(m, vals, vdev[:aft.cap])
            x = torch.from_numpy(feat)
            with torch.no_grad():
                a32 = c(x).double().numpy().reshape(-1)
                a64 = copy.deepcopy(c).double()(x.double()).numpy().reshape(-1)
            v32[sel], v64[sel] = a32[sel], a64[sel]
        term = reward != 0
        oc = np.where(feat[:, 197] > 0.5, -1.0, 1.0) * reward
        v32, v64 = np.where(term, oc, v32), np.where(term, oc, v64)
        if aft.cap:
            pick_play, pick_row = env2.pick_turn(scored, vdev, "white", eps, None if eps is None else TAG + k, PICK_SEED)
            pick_play, pick_row, vsc = np_(pick_play), np_(pick_row), np_(vdev)
        for e in range(B):
            got = out["play"][k, e]
            val = out["value"][k, e]
            g = gb if player[e] == -1 else gw
            if g is None:
                J["random"] += 1
                assert np.array_equal(got, rand_play[e]) and np.isnan(val), f"ply {k} env {e}: random ply"
                continue
            r0, r1 = int(offs[e]), int(offs[e + 1])
            J["most_rows"] = max(J["most_rows"], r1 - r0)
            J["above_256"] += int(r1 - r0 > 256)
            if r1 == r0:
                J["norow"] += 1
                assert (got == -1).all() and np.isnan(val), f"ply {k} env {e}: no row"
                continue
            hit = np.nonzero((plays[r0:r1] == got[None]).all((1, 2)))[0]
            assert len(hit) == 1, f"ply {k} env {e}: play {got.tolist()} is not a row"
            j = int(hit[0])
            sign = -1.0 if player[e] == -1 else 1.0
            x64 = v64[r0:r1] * sign
            J["e32"] = max(J["e32"], float(np.abs(v32[r0:r1] - v64[r0:r1]).max()))
            J["mag"] = max(J["mag"], float(np.abs(v64[r0:r1]).max()))
            J["verr"].append(abs(float(val) - float(v64[r0 + j])))
            J["value_bits_equal"] += int(np.float32(val).view(np.uint32) == np.float32(vsc[r0 + j]).view(np.uint32))
            J["play_equals_pick"] += int(np.array_equal(got, pick_play[e]))
            J["terminal_pick"] += int(term[r0 + j])
            explore = False
            if eps_q is not None:
                r = O.philox(((TAG + k) & M32, e, 0, 5), (PICK_SEED & M32, PICK_SEED >> 32))
                explore = r[0] < eps_q
            if explore:
                J["explored"] += 1
                J["explore_ordinal_64"] += int(mulhi(r[1], r1 - r0) >= 64)  # the drawn row is not in the first chunk
                assert np.array_equal(got, pick_play[e]) and pick_row[e] == r0 + j, f"ply {k} env {e}: explore"
                continue
            J["greedy"] += 1
            J["greedy_above_64"] += int(r1 - r0 > 64)  # a second 64-row chunk
            jb = int(np.argmax(x64))
            rest = np.delete(x64, jb)
            J["gap"].append(float(x64[jb] - rest.max()) if len(rest) else np.inf)
            J["is_best"].append(j == jb)
            J["short"].append(float(x64[jb] - x64[j]))
        _, rew, tm, tr, _ = env2.step(bufs["play"][k])
        assert np.array_equal(np_(rew), out["reward"][k]), f"ply {k}: reward"
        assert np.array_equal(np_(tm), out["terminated"][k]) and np.array_equal(np_(tr), out["truncated"][k]), f"ply {k}"
        J["resets"] += int(((np_(tm) != 0) | (np_(tr) != 0)).sum())
    return J


def run_case(B, plies, white, black=SAME, eps=None, max_steps=1000, state=None, what="", scratch_waves=None):
    env, env2 = make_env(B, max_steps, state), make_env(B, max_steps, state)
    gw, cw = twins(white, env.device)
    gb, cb = (gw, cw) if black is SAME else twins(black, env.device)
    scratch = None if scratch_waves is None else env.turn_value_rollout_scratch(scratch_waves)
    bufs = env.turn_value_rollout(plies, gw, gb, epsilon=eps, tag=None if eps is None else TAG, seed=PICK_SEED,
                                  scratch=scratch)
    J = replay(env2, bufs, plies, gw, cw, gb, cb, eps, max_steps)
    assert_same_env(env, env2)
    n = J["greedy"] + J["explored"]
    print(f"{what}: value bit-equal to scored_turn_afterstates() on {J['value_bits_equal']} of {n} plies, play equal to "
          f"pick_turn()'s on {J['play_equals_pick']} of {n}")
    judge(J, what)
    env.close()
    env2.close()
    return J, bufs


@pytest.mark.parametrize("B,plies,spec", [(1, 1, H80), (65, 7, H1), (257, 7, H128), (257, 1, H17), (1, 7, H17),
                                          (65, 1, H128), (65, 7, H80), (257, 1, H1)])
def test_replay_against_the_existing_calls(B, plies, spec):
    J, _ = run_case(B, plies, spec, what=f"B {B} plies {plies} H {spec[0]}")
    assert J["greedy"] + J["norow"] == B * plies


def test_two_different_nets():
    J, _ = run_case(65, 7, H80, H17, what="H 80 white, H 17 black")
    assert J["greedy"] > 400


def test_black_random():
    J, _ = run_case(65, 7, H80, None, what="black random")
    assert J["random"] > 150 and J["greedy"] > 150


def test_white_random():
    J, _ = run_case(65, 3, None, H17, what="white random")
    assert J["random"] > 60 and J["greedy"] > 60


def test_epsilon():
    J, _ = run_case(65, 7, H80, eps=0.3, what="epsilon 0.3")
    assert J["explored"] > 80 and J["greedy"] > 200


def test_truncation_and_reset_inside_a_launch():
    J, _ = run_case(65, 7, H80, max_steps=5, what="max_episode_steps 5")
    assert J["resets"] >= 65


def test_terminal_rows_are_picked_and_the_reset_happens_mid_launch():
    b, o, f, p = endgames()  # one ply from winning: both colours, 1 and 2 points
    state = tuple(np.ascontiguousarray(np.concatenate([a, a])) for a in (b, o, f, p))
    J, _ = run_case(8, 3, H80, H17, state=state, what="endgames")
    assert J["terminal_pick"] >= 8 and J["resets"] >= 8


def test_a_level_past_the_chip_tier_walks_in_the_slab():
    """big_state() (2,065 rows under 1-1, past the 256-node tier) on exactly
    the envs of a B = 257 batch whose first roll is 1-1; every other env's
    bits are those it has in the batch without big_state()."""
    B, plies = 257, 2
    probe = make_env(B)
    first = np_(probe.dice())
    base = {k: np_(v) for k, v in probe.get_state().items()}
    probe.close()
    ones = np.flatnonzero((first == 1).all(1))
    assert len(ones) >= 1, "no env of the batch rolls 1-1 first: choose another seed"
    big = big_state()
    board, off, ft, player = (base[k].copy() for k in ("board", "off", "first_turn", "player"))
    board[ones], off[ones], ft[ones], player[ones] = big["board"], big["off"], big["ft"], big["player"]
    J, with_big = run_case(B, plies, H80, H17, state=(board, off, ft, player), what="big_state on the 1-1 envs")
    assert J["most_rows"] == BIG_ROWS
    plain = make_env(B)
    gw, _ = twins(H80, plain.device)
    gb, _ = twins(H17, plain.device)
    without = plain.turn_value_rollout(plies, gw, gb, seed=PICK_SEED)
    others = np.setdiff1d(np.arange(B), ones)
    for k in KEYS:
        a, b = (np.ascontiguousarray(np_(x[k])[:, others]).view(np.uint8) for x in (with_big, without))
        assert np.array_equal(a, b), k
    plain.close()


def test_three_pieces_of_scratch_give_the_same_bits():
    """B = 65 over 3 waves (about 22 envs a wave) = 65 waves."""
    B, plies = 65, 7
    a, b = make_env(B, 5), make_env(B, 5)
    gw, _ = twins(H80, a.device)
    gb, _ = twins(H17, a.device)
    few = a.turn_value_rollout(plies, gw, gb, epsilon=0.3, tag=TAG, seed=PICK_SEED,
                               scratch=a.turn_value_rollout_scratch(3))
    all_ = b.turn_value_rollout(plies, gw, gb, epsilon=0.3, tag=TAG, seed=PICK_SEED,
                                scratch=b.turn_value_rollout_scratch(65))
    assert_same_bufs(few, all_)
    assert_same_env(a, b)
    assert 1 <= a.turn_value_rollout_waves() <= 64 * 1024
    a.close()
    b.close()


def test_c_call_with_a_padded_weight_stride():
    """ld_w1t = H + 4: the same bits as the packed net."""
    from gym_narde import _lib

    B, plies = 65, 7
    env, ref = make_env(B), make_env(B)
    g, _ = twins(H17, env.device)
    want = ref.turn_value_rollout(plies, g)
    H = g.hidden
    w1t = torch.full((198, H + 4), 1e9, dtype=torch.float32, device=env.device)  # a read past H would show
    w1t[:, :H] = g.l1.weight.detach().t()
    mlp = _lib.ValueMlp(w1t.data_ptr(), H + 4, g.l1.bias.data_ptr(), g.l2.weight.data_ptr(), g.l2.bias.data_ptr(), H,
                        g.struct().hidden_act, g.struct().out_act)
    bufs = env.turn_value_rollout_buffers(plies)
    scratch = env.turn_value_rollout_scratch()
    env.handle.call("narde_turn_value_rollout", plies, ctypes.byref(mlp), ctypes.byref(mlp), None, PICK_SEED, None,
                    *(_lib.ptr(bufs[k]) for k in KEYS), _lib.ptr(scratch), scratch.numel(), env._s())
    assert_same_bufs(bufs, want)
    assert_same_env(env, ref)
    env.close()
    ref.close()


def test_loop_carry_and_determinism():
    """One 7-ply launch = seven 1-ply launches with tag + k by hand = the
    same launch on a fresh env: state, stats, every output and t."""
    B, plies = 65, 7
    g, _ = twins(H80, torch.device("cuda:0"))
    gb, _ = twins(H17, torch.device("cuda:0"))
    a, b, c = make_env(B, 5), make_env(B, 5), make_env(B, 5)
    one = a.turn_value_rollout(plies, g, gb, epsilon=0.3, tag=TAG, seed=PICK_SEED)
    again = c.turn_value_rollout(plies, g, gb, epsilon=0.3, tag=TAG, seed=PICK_SEED)
    steps = [b.turn_value_rollout(1, g, gb, epsilon=0.3, tag=TAG + k, seed=PICK_SEED) for k in range(plies)]
    for k in KEYS:
        whole = np_(one[k]).view(np.uint8)
        assert np.array_equal(whole, np_(again[k]).view(np.uint8)), k
        assert np.array_equal(whole, np.concatenate([np_(s[k]) for s in steps]).view(np.uint8)), k
    assert_same_env(a, b)
    assert_same_env(a, c)
    assert a.ply == plies
    for e in (a, b, c):
        e.close()


def test_graph_replay():
    """A captured 3-ply launch with the caller's scratch, replayed once,
    continues the games: t lives in device state.  One kernel node."""
    B = 65
    g, _ = twins(H80, torch.device("cuda:0"))
    g.pack()
    a, b = make_env(B), make_env(B)
    bufs = a.turn_value_rollout_buffers(3)
    scratch = a.turn_value_rollout_scratch()
    a.turn_value_rollout(3, g, bufs=bufs, scratch=scratch)  # warm-up: plies 0..2
    first = {k: v.clone() for k, v in bufs.items()}
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            a.turn_value_rollout(3, g, bufs=bufs, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()  # plies 3..5
    torch.cuda.synchronize()
    want = b.turn_value_rollout(6, g)
    for k in KEYS:
        got = np.concatenate([np_(first[k]), np_(bufs[k])])
        assert np.array_equal(got.view(np.uint8), np_(want[k]).view(np.uint8)), k
    assert_same_env(a, b)
    a.close()
    b.close()


def test_play_turn_match_against_random_finishes_games():
    from gym_narde.value_play import play_turn_match

    env = make_env(64)
    g, _ = twins(H80, env.device)
    res = play_turn_match(env, g, None, 300)
    assert res["games"] > 0 and res["points_a"] + res["points_b"] > 0
    # the second launch's totals are the env's stats() now; the first's by hand
    ep, pw, pb = (int(x) for x in np_(env.stats()).sum(0))
    assert res["by_colour"]["a_black"] == {"games": ep, "points_a": pb, "points_b": pw}
    env.close()
    env = make_env(64)  # (a reset's opening rolls depend on how many came before it)
    env.reset()
    env.turn_value_rollout(300, g, None)
    ep, pw, pb = (int(x) for x in np_(env.stats()).sum(0))
    assert res["by_colour"]["a_white"] == {"games": ep, "points_a": pw, "points_b": pb}
    assert res["games"] == sum(v["games"] for v in res["by_colour"].values())
    assert res["points_a"] == sum(v["points_a"] for v in res["by_colour"].values())
    assert res["points_b"] == sum(v["points_b"] for v in res["by_colour"].values())
    env.close()


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_examples_under_full4(tmp_path, capsys):
    path = str(tmp_path / "agent.pt")
    _example("train_value_agent").main(envs=64, plies=20, out=path, device="cuda:0", rules="full4")
    res = _example("eval_value_agents").main(path, None, envs=64, plies=150, device="cuda:0", rules="full4")
    assert res["games"] > 0 and "against random play" in capsys.readouterr().out
    res2 = _example("eval_value_agents").main(path, path, envs=64, plies=150, device="cuda:0", rules="full4")
    assert res2["games"] > 0
    play = _example("play_value_agent").main
    ep, w, b = play(envs=64, plies=150, device="cuda:0", rules="full4", one_launch=True)
    ep2, w2, b2 = play(envs=64, plies=150, device="cuda:0", rules="full4", fused=True)
    assert (ep, w, b) == (ep2, w2, b2) and ep > 0  # the same games as the per-ply loop


def test_python_errors():
    env = make_env(4)
    g, _ = twins(H17, env.device)
    with pytest.raises(TypeError):
        env.turn_value_rollout(2, torch.nn.Linear(198, 1).to(env.device))
    with pytest.raises(ValueError):
        env.turn_value_rollout(2, None, None)
    with pytest.raises(ValueError):
        env.turn_value_rollout(0, g)
    with pytest.raises(ValueError):
        env.turn_value_rollout(2, g, epsilon=0.1)
    with pytest.raises(ValueError):
        env.turn_value_rollout(2, copy.deepcopy(g).cpu())
    with pytest.raises(ValueError):
        env.turn_value_rollout(3, g, bufs=env.turn_value_rollout_buffers(2))
    with pytest.raises(ValueError):
        env.turn_value_rollout(2, g, scratch=torch.empty(100, dtype=torch.uint8, device=env.device))
    env.close()
    ref2 = make_env(4, rules="ref2")
    with pytest.raises(ValueError):
        ref2.turn_value_rollout(2, g)
    from gym_narde.value_play import play_turn_match

    with pytest.raises(ValueError):
        play_turn_match(ref2, g, None, 2)
    ref2.close()
