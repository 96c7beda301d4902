"""Afterstates scored by the built-in value MLP on the GPU (k_aft_fill_scored,
k_turn_fill_scored, k_turn_overflow_scored through
VecNardeEnv.scored_afterstates / scored_turn_afterstates and the fused
ValuePlayer): the structural outputs bit for bit against the plain calls, the
values against torch's float64 evaluation of ValueMLP.forward on the plain
call's feat within tol = 8 x E, E = max |torch-fp32 - torch-fp64| on the same
rows (tests/test_value_cpu.py states the argument), terminal rows exact.
"""
import copy

import numpy as np
import pytest

import turn_afterstates_ref as R
from test_afterstates_cpu import golden_states, reference_afterstates
from test_value_cpu import TOL_FACTOR, make_net, torch_values

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import _env, _pick_ref, np_  # noqa: E402
from test_gpu_afterstates import _first  # noqa: E402

KEYS = ("board", "off", "ft", "player", "dice")
SIGMOID80 = (80, "sigmoid", "sigmoid", 1)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def case():
    st = golden_states()
    return st, reference_afterstates(*st)


@pytest.fixture(scope="module")
def turn_case():
    """tests/test_gpu_turn_afterstates.py's states: B = 1,003, the 2,065-row
    position at envs 0, 500 and B - 1 (the fast path, the LDS overflow tier
    and the slab tier)."""
    B = 1003
    sp = R.selfplay_states()
    parts = [R.edge_states(), R.start_states()]
    n = B - sum(len(p["player"]) for p in parts)
    parts.append({k: sp[k][::2][:n] for k in KEYS})
    st = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in KEYS}
    big = R.big_state()
    for e in (0, 500, B - 1):
        for k in KEYS:
            st[k][e] = big[k]
    return st


def nets(spec, device):
    """The net on the device and its CPU twin (the reference)."""
    cpu = make_net(*spec)
    return copy.deepcopy(cpu).to(device), cpu


def expected(cpu_net, feat, reward, perspective):
    """(torch-fp64 values with the terminal rows' outcomes, E, terminal mask)."""
    feat, reward = np_(feat), np_(reward)
    if len(reward) == 0:
        return np.zeros(0), 0.0, np.zeros(0, bool)
    want, E = torch_values(cpu_net, feat)
    term = reward != 0
    r = reward.astype(np.float64)
    want = np.where(term, np.where((feat[:, 197] > 0.5) & (perspective == "white"), -r, r), want)
    return want, E, term


def check_values(values, want, E, term, what=""):
    got = np_(values).astype(np.float64)
    assert got.shape == want.shape
    err = float(np.abs(got[~term] - want[~term]).max()) if (~term).any() else 0.0
    print(f"{what}: E = {E:.3e}, max error = {err:.3e} = {err / max(E, 1e-30):.2f} E")
    assert err <= TOL_FACTOR * E, (what, err, TOL_FACTOR * E)
    assert np.array_equal(got[term], want[term])  # terminal rows: exact


@pytest.mark.parametrize("spec", [SIGMOID80, (1, "relu", "none", 3), (65, "relu", "tanh", 4), (128, "tanh", "none", 2)],
                         ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
@pytest.mark.parametrize("B", [1, 65, 1003])
def test_ref2_rows_and_values(case, B, spec):
    st, ref = _first(case, B)
    env = _env(st)
    net, cpu = nets(spec, env.device)
    plain = env.afterstates(dice=st[4])
    cnt = np.diff(np_(plain.offsets))
    assert cnt.max() == 82 and (B < 1003 or (cnt == 0).any())
    for perspective in ("white", "mover"):
        aft, values = env.scored_afterstates(net, dice=st[4], perspective=perspective)
        assert aft.feat is None and aft.obs is None and aft.cap == plain.cap and values.shape == (plain.cap,)
        for k in ("offsets", "row_env", "codes", "reward"):
            assert torch.equal(getattr(aft, k), getattr(plain, k)), k
        want, E, term = expected(cpu, plain.feat, plain.reward, perspective)
        check_values(values, want, E, term, f"ref2 B={B} {spec[:3]} {perspective}")
        if B == 1003:  # both colours end games here: the sign rule is exercised
            black = np_(plain.feat)[:, 197] > 0.5
            assert (term & black).any() and (term & ~black).any()
    env.close()


def test_ref2_whole_case(case):
    """All 4,004 states: the 144 envs with no row, terminal rows of reward 1
    and 2 for both colours."""
    st, ref = case
    env = _env(st)
    net, cpu = nets(SIGMOID80, env.device)
    plain = env.afterstates(dice=st[4])
    rew, black = np_(plain.reward), np_(plain.feat)[:, 197] > 0.5
    assert (np.diff(np_(plain.offsets))[:4001] == 0).sum() == 144
    assert all(((rew == r) & (black == b)).any() for r in (1, 2) for b in (False, True))
    for perspective in ("white", "mover"):
        aft, values = env.scored_afterstates(net, dice=st[4], perspective=perspective)
        for k in ("offsets", "row_env", "codes", "reward"):
            assert torch.equal(getattr(aft, k), getattr(plain, k)), k
        want, E, term = expected(cpu, plain.feat, plain.reward, perspective)
        check_values(values, want, E, term, f"ref2 B=4004 {perspective}")
    env.close()


def test_cap_cuts_values_not_offsets(case):
    from gym_narde.vector import Afterstates

    st, ref = _first(case, 1003)
    env = _env(st)
    net, cpu = nets(SIGMOID80, env.device)
    plain = env.afterstates(dice=st[4])
    o = np_(plain.offsets)
    total = int(o[-1])
    e = int(np.nonzero(np.diff(o) >= 5)[0][200])
    cap = int(o[e]) + 2
    assert o[e] < cap < o[e + 1] and cap < total
    dev = env.device
    out = Afterstates(torch.zeros(1004, dtype=torch.int32, device=dev),
                      torch.full((total,), -7, dtype=torch.int32, device=dev),
                      torch.full((total, 2), -7, dtype=torch.int16, device=dev), None, None,
                      torch.full((total,), -7, dtype=torch.int8, device=dev), cap)
    vals = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    aft, values = env.scored_afterstates(net, dice=st[4], out=(out, vals))
    assert aft.cap == cap and values.shape == (cap,)
    assert np.array_equal(np_(aft.offsets), o) and int(o[-1]) == total > cap  # the true counts
    for a in (aft.row_env, aft.codes, aft.reward, vals):
        assert (np_(a)[cap:] == -7).all()
    for k in ("row_env", "codes", "reward"):
        assert torch.equal(getattr(aft, k)[:cap], getattr(plain, k)[:cap]), k
    want, E, term = expected(cpu, plain.feat[:cap], plain.reward[:cap], "white")
    check_values(vals[:cap], want, E, term, "ref2 cap")
    # cap = 0: the counts alone
    aft0, v0 = env.scored_afterstates(net, dice=st[4], cap=0)
    assert aft0.cap == 0 and v0.shape == (0,) and np.array_equal(np_(aft0.offsets), o)
    env.close()


def test_full4_rows_and_values(turn_case):
    st = turn_case
    env = _env([st[k] for k in KEYS], rules="full4")
    net, cpu = nets(SIGMOID80, env.device)
    plain = env.turn_afterstates(dice=st["dice"])
    cnt = np.diff(np_(plain.offsets))
    assert all(cnt[e] == R.BIG_ROWS for e in (0, 500, 1002)) and (cnt == 0).any() and (np_(plain.reward) != 0).any()
    for perspective in ("white", "mover"):
        aft, values = env.scored_turn_afterstates(net, dice=st["dice"], perspective=perspective)
        assert aft.feat is None and aft.cap == plain.cap
        for k in ("offsets", "row_env", "play", "reward"):
            assert torch.equal(getattr(aft, k), getattr(plain, k)), k
        want, E, term = expected(cpu, plain.feat, plain.reward, perspective)
        check_values(values, want, E, term, f"full4 {perspective}")
    # a cap inside the mid-wave heavy env's rows (the overflow path): nothing at or past it is touched
    from gym_narde.vector import TurnAfterstates

    o = np_(plain.offsets)
    total, cap = int(o[-1]), int(o[500]) + 701
    dev = env.device
    out = TurnAfterstates(torch.zeros(1004, dtype=torch.int32, device=dev),
                          torch.full((total,), -7, dtype=torch.int32, device=dev),
                          torch.full((total, 4, 2), -7, dtype=torch.int8, device=dev), None, None,
                          torch.full((total,), -7, dtype=torch.int8, device=dev), cap)
    vals = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    aft, values = env.scored_turn_afterstates(net, dice=st["dice"], out=(out, vals))
    assert aft.cap == cap and o[500] < cap < o[501] and np.array_equal(np_(aft.offsets), o)
    for a in (aft.row_env, aft.play, aft.reward, vals):
        assert (np_(a)[cap:] == -7).all()
    want, E, term = expected(cpu, plain.feat[:cap], plain.reward[:cap], "white")
    check_values(vals[:cap], want, E, term, "full4 cap")
    env.close()


@pytest.mark.parametrize("rules", ["ref2", "full4"])
def test_value_player_fused_against_unfused(rules):
    from gym_narde.value_play import ValuePlayer
    from gym_narde.vector import VecNardeEnv

    B = 257
    env = VecNardeEnv(B, device="cuda:0", seed=2026, rules=rules)
    net, cpu = nets(SIGMOID80, env.device)
    player = ValuePlayer(env, net, perspective="white")
    assert player.fused and not ValuePlayer(env, torch.nn.Sequential(), fused=None).fused
    expand, scored, pick = ((env.turn_afterstates, env.scored_turn_afterstates, env.pick_turn) if env.full else
                            (env.afterstates, env.scored_afterstates, env.pick_afterstate))
    env.selfplay(60)  # into the middle game and the bear-off
    for ply in range(30):
        black = np_(env.get_state()["player"]) == -1
        dice = env.dice()
        plain = expand(dice)
        aft0, v0 = scored(net, dice, perspective="white")
        a0, r0 = pick(aft0, v0, "white")
        obs, reward, term, trunc, info, aft, values, actions = player.step()
        # the wiring: the step's pick is pick_*'s on the kernel's values, which are the same on every call
        assert aft.feat is None and torch.equal(values, v0) and torch.equal(info["row"], r0)
        assert torch.equal(actions, a0) and torch.equal(aft.offsets, plain.offsets)
        o = np_(aft.offsets)
        assert np.array_equal(np_(r0), _pick_ref(o, aft.cap, np_(v0), black, "white")), ply
        # the row played is, by torch-fp64, within 2 tol of the env's best -- every env
        want, E, _ = expected(cpu, plain.feat, plain.reward, "white")
        row = np_(r0).astype(np.int64)
        for e in np.nonzero(row >= 0)[0]:
            seg = want[o[e]:o[e + 1]]
            best = seg.min() if black[e] else seg.max()
            assert abs(want[row[e]] - best) <= 2 * TOL_FACTOR * E, (ply, int(e))
        assert ((row >= 0) == (np.diff(o) > 0)).all()
    # cap given: the arrays hold cap rows, the pick is the kernel's values' own
    cap = B * (96 if env.full else 40)
    black = np_(env.get_state()["player"]) == -1
    _, _, _, _, info, aft, values, _ = ValuePlayer(env, net, perspective="white", cap=cap).step()
    assert aft.cap == cap and values.shape == (cap,) and int(aft.offsets[B]) <= cap
    assert np.array_equal(np_(info["row"]), _pick_ref(np_(aft.offsets), cap, np_(values), black, "white"))
    # fused=False: the dense path, as with any other module
    slow = ValuePlayer(env, net, perspective="white", fused=False)
    assert slow.step()[5].feat is not None
    env.close()


def test_graph_replay_reads_the_live_weights():
    """scored_afterstates(cap) + pick + step captured once; l1.weight changed
    in place and pack()ed between two replays: each replay's values are
    torch-fp64's for the weights live at that replay."""
    from gym_narde.vector import Afterstates, VecNardeEnv

    B, cap = 257, 257 * 40
    env = VecNardeEnv(B, device="cuda:0", seed=99)
    dev = env.device
    net, cpu = nets(SIGMOID80, dev)
    env.selfplay(25)
    out = Afterstates(torch.zeros(B + 1, dtype=torch.int32, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev),
                      torch.zeros((cap, 2), dtype=torch.int16, device=dev), None, None,
                      torch.zeros(cap, dtype=torch.int8, device=dev), cap)
    vals = torch.zeros(cap, dtype=torch.float32, device=dev)
    net.pack()
    torch.cuda.synchronize()

    def ply():
        aft, values = env.scored_afterstates(net, out=(out, vals))
        actions, row = env.pick_afterstate(aft, values, perspective="white")
        env.step(actions)
        return row

    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g_row = ply()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for rep in range(2):
        plain = env.afterstates()  # this replay's rows, before it plays one
        black = np_(env.get_state()["player"]) == -1
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        n = plain.cap
        assert 0 < n <= cap and torch.equal(out.offsets, plain.offsets)
        want, E, term = expected(cpu, plain.feat, plain.reward, "white")
        check_values(vals[:n], want, E, term, f"replay {rep}")
        assert np.array_equal(np_(g_row), _pick_ref(np_(out.offsets), cap, np_(vals), black, "white"))
        # new weights, in place on both twins; pack() hands them to the next replay
        torch.manual_seed(100 + rep)
        delta = torch.randn(80, 198) * 0.5
        with torch.no_grad():
            cpu.l1.weight.add_(delta)
            net.l1.weight.add_(delta.to(dev))
        net.pack()
    env.close()
