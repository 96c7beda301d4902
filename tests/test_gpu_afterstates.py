"""Afterstate expansion and value-greedy play on the GPU (k_aft_count,
k_aft_scan, k_aft_fill, k_aft_pick through VecNardeEnv.afterstates /
pick_afterstate and gym_narde.value_play.ValuePlayer), every output bit for
bit against the restatement over the C oracle of
tests/test_afterstates_cpu.py, and against narde_step itself.
"""
import numpy as np
import pytest

import oracle as O
from test_afterstates_cpu import golden_states, reference_afterstates

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import _check_pick, _env, _equal, _pick_ref, _scored_ply, np_  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def case():
    """golden steps [::11] + the three rows with 82 / 80 / 79 afterstates
    (4,004 states) and their reference rows, computed once and left alone."""
    st = golden_states()
    return st, reference_afterstates(*st)


def _take(case, idx):
    """The states idx of the case and their reference rows."""
    st, ref = case
    idx = np.asarray(idx)
    o = ref["offsets"]
    rows = np.concatenate([np.arange(o[i], o[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    cnt = np.array([o[i + 1] - o[i] for i in idx], np.int64)
    sub = {k: ref[k][rows] for k in ("codes", "board", "off", "player", "obs", "reward", "feat", "terminated")}
    sub["offsets"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    sub["row_env"] = np.repeat(np.arange(len(idx)), cnt).astype(np.int32)
    return tuple(a[idx] for a in st), sub


def _first(case, B):
    """B states holding the large golden rows (the case's last three)."""
    n = case[0][0].shape[0]
    big = [n - 3, n - 2, n - 1]
    return _take(case, big[:B] if B <= 3 else list(range(B - 3)) + big)


@pytest.mark.parametrize("B", [1, 65, 1003, 4004])
def test_rows_equal_the_restatement(case, B):
    """B = 1, one wave plus one lane, 1,003 and the whole case: every output,
    in order, bit for bit."""
    st, want = _first(case, B)
    assert np.diff(want["offsets"]).max() >= 79
    env = _env(st)
    aft = env.afterstates(dice=st[4], obs=True)
    assert aft.cap == int(want["offsets"][-1]) and aft.feat.shape == (aft.cap, 198)
    _equal(aft, want)
    # feat=False / obs=False leave those arrays out, the rest unchanged
    lean = env.afterstates(dice=st[4], feat=False)
    assert lean.feat is None and lean.obs is None
    assert np.array_equal(np_(lean.codes), want["codes"]) and np.array_equal(np_(lean.offsets), want["offsets"])
    env.close()


def test_offsets_carry_across_scan_tiles(case):
    """B = 40,040 (the case ten times over): the offsets scan works in tiles
    of 32,768 envs and carries the running total from one to the next."""
    st, want = case
    rep = 10
    env = _env(tuple(np.tile(a, (rep,) + (1,) * (a.ndim - 1)) for a in st))
    aft = env.afterstates(dice=np.tile(st[4], (rep, 1)), feat=False)
    cnt = np.tile(np.diff(want["offsets"]), rep)
    assert np.array_equal(np_(aft.offsets), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
    assert np.array_equal(np_(aft.codes), np.tile(want["codes"], (rep, 1)))
    assert np.array_equal(np_(aft.row_env), np.repeat(np.arange(cnt.size), cnt).astype(np.int32))
    env.close()


def test_cap_cuts_rows_not_offsets(case):
    st, want = _first(case, 1003)
    env = _env(st)
    total = int(want["offsets"][-1])
    o = want["offsets"]
    # a cut inside an env's rows, at an odd row (a feature row is 792 B: the
    # run then ends 8 B into a 16-B piece)
    e = int(np.nonzero(np.diff(o) >= 5)[0][200])
    cap = int(o[e]) + 2 + (int(o[e]) % 2 == 0)
    assert cap % 2 == 1 and o[e] < cap < o[e + 1] and cap < total
    from gym_narde.vector import Afterstates

    dev = env.device
    out = Afterstates(torch.zeros(1004, dtype=torch.int32, device=dev),
                      torch.full((total,), -7, dtype=torch.int32, device=dev),
                      torch.full((total, 2), -7, dtype=torch.int16, device=dev),
                      torch.full((total, 198), -7.0, dtype=torch.float32, device=dev),
                      torch.full((total, 24), -7, dtype=torch.int32, device=dev),
                      torch.full((total,), -7, dtype=torch.int8, device=dev), cap)
    aft = env.afterstates(dice=st[4], out=out)
    assert aft.cap == cap
    _equal(aft, want, rows=cap)  # offsets: the true counts
    assert int(np_(aft.offsets)[-1]) == total > cap
    for a in (aft.row_env, aft.codes, aft.feat, aft.obs, aft.reward):
        assert (np_(a)[cap:] == -7).all()
    # pick ignores the cut rows: the best value sits in them
    values = torch.zeros(total, dtype=torch.float32, device=dev)
    values[cap:] = 9.0
    black = st[3] == -1
    rows = _check_pick(env, aft, values, black, "mover", want["codes"])
    assert rows.max() < cap and rows[e] == o[e] and (rows[e + 1:] == -1).all()
    env.close()


def test_device_dice_equal_given_dice():
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(1003, device="cuda:0", seed=77)
    env.selfplay(37)
    a = env.afterstates(obs=True)
    b = env.afterstates(dice=env.dice(), obs=True)
    assert a.cap == b.cap and a.cap > 1003
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    # and equal to the restatement on the env's own states and dice
    s = env.get_state()
    want = reference_afterstates(np_(s["board"]), np_(s["off"]), np_(s["first_turn"]), np_(s["player"]), np_(env.dice()))
    want["row_env"] = np.repeat(np.arange(1003), np.diff(want["offsets"])).astype(np.int32)
    _equal(a, want)
    env.close()


def test_step_carries_out_the_row(case):
    """A random row per env, stepped: the env's observation, obs, reward and
    terminated are the row's."""
    st, want = _first(case, 1003)
    env = _env(st)
    aft = env.afterstates(dice=st[4], obs=True)
    o = np_(aft.offsets).astype(np.int64)
    cnt = np.diff(o)
    rng = np.random.default_rng(5)
    has = cnt > 0
    row = o[:-1] + (rng.random(1003) * cnt).astype(np.int64)
    codes = np.where(has[:, None], np_(aft.codes)[np.minimum(row, aft.cap - 1)], 0).astype(np.int16)
    obs, reward, term, _, info = env.step(codes, st[4])
    feat = np_(env.tesauro198())
    r = row[has]
    assert has.sum() > 900 and (np_(aft.reward)[r] != 0).any()
    assert np.array_equal(feat[has].view(np.uint32), np_(aft.feat)[r].view(np.uint32))
    assert np.array_equal(np_(obs)[has], np_(aft.obs)[r])
    assert np.array_equal(np_(reward)[has], np_(aft.reward)[r].astype(np.int32))
    assert np.array_equal(np_(term)[has] != 0, np_(aft.reward)[r] != 0)
    assert np.array_equal(np_(info["actions"])[has], codes[has])
    env.close()


@pytest.mark.parametrize("perspective", ["white", "mover"])
def test_pick_equals_torch_segments(case, perspective):
    st, want = _first(case, 1003)
    env = _env(st)
    aft = env.afterstates(dice=st[4])
    rng = np.random.default_rng(9)
    v = rng.integers(0, 4, aft.cap).astype(np.float32) / 4 - 0.5  # four levels: ties everywhere
    v[rng.random(aft.cap) < 0.01] = np.nan
    black = st[3] == -1
    assert black.any() and (~black).any() and (np.diff(want["offsets"]) == 0).any()
    values = torch.from_numpy(v).to(env.device)
    rows = _check_pick(env, aft, values, black, perspective, want["codes"])
    assert (rows == -1).sum() == (np.diff(want["offsets"]) == 0).sum()
    # a strided (R, 1) column of a wider tensor
    wide = torch.zeros((aft.cap, 3), dtype=torch.float32, device=env.device)
    wide[:, 1] = values
    a2, r2 = env.pick_afterstate(aft, wide[:, 1:2], perspective=perspective)
    assert np.array_equal(np_(r2), rows)
    env.close()


def test_pick_explores_uniformly_over_the_rows(case):
    st, want = _first(case, 1003)
    env = _env(st)
    aft = env.afterstates(dice=st[4])
    values = torch.zeros(aft.cap, dtype=torch.float32, device=env.device)
    seed, tag = 0x1234567890, 41
    eps = torch.tensor(1.0, dtype=torch.float32, device=env.device)
    tg = torch.tensor(tag, dtype=torch.int64, device=env.device)
    actions, row = env.pick_afterstate(aft, values, epsilon=eps, tag=tg, seed=seed)
    o = want["offsets"].astype(np.int64)
    exp = np.full(1003, -1, np.int64)
    for e in range(1003):
        cnt = int(o[e + 1] - o[e])
        if cnt:
            r = O.philox((tag, e, 0, 5), (seed & 0xFFFFFFFF, seed >> 32))
            exp[e] = o[e] + ((r[1] * cnt) >> 32)
    assert np.array_equal(np_(row), exp)
    assert np.array_equal(np_(actions), np.where((exp >= 0)[:, None], want["codes"][np.maximum(exp, 0)], 0))
    # epsilon 0: greedy (all values tie: the first row)
    actions, row = env.pick_afterstate(aft, values, epsilon=0.0, tag=tag, seed=seed)
    assert np.array_equal(np_(row), np.where(np.diff(o) > 0, o[:-1], -1))
    env.close()


def test_graph_capture_equals_eager():
    """afterstates(cap) + pick + step captured once (linear) and replayed: no
    allocation or synchronise inside the call."""
    from gym_narde.vector import Afterstates, VecNardeEnv

    B, cap, seed = 257, 257 * 40, 99
    envs = [VecNardeEnv(B, device="cuda:0", seed=seed) for _ in range(2)]
    dev = envs[0].device
    w = torch.linspace(-1, 1, 198, device=dev)
    score = lambda feat: (feat * w).sum(1)  # noqa: E731
    mk = lambda: Afterstates(torch.zeros(B + 1, dtype=torch.int32, device=dev),  # noqa: E731
                             torch.zeros(cap, dtype=torch.int32, device=dev),
                             torch.zeros((cap, 2), dtype=torch.int16, device=dev),
                             torch.zeros((cap, 198), dtype=torch.float32, device=dev), None,
                             torch.zeros(cap, dtype=torch.int8, device=dev), cap)
    for e in envs:
        e.selfplay(25)
    outs = [mk(), mk()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g_actions, g_row = _scored_ply(envs[0], outs[0], score)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e_actions, e_row = _scored_ply(envs[1], outs[1], score)
        torch.cuda.synchronize()
        assert int(outs[1].offsets[B]) <= cap
        assert torch.equal(g_actions, e_actions) and torch.equal(g_row, e_row)
        assert torch.equal(outs[0].offsets, outs[1].offsets)
    a, b = envs[0].get_state(), envs[1].get_state()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for e in envs:
        e.close()


def test_value_player_plays_its_own_argmax():
    from gym_narde.value_play import ValuePlayer
    from gym_narde.vector import VecNardeEnv

    B = 257
    env = VecNardeEnv(B, device="cuda:0", seed=2026)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(198, 80), torch.nn.Sigmoid(), torch.nn.Linear(80, 1),
                              torch.nn.Sigmoid()).to(env.device)
    player = ValuePlayer(env, net, perspective="white")
    env.selfplay(60)  # into the middle game and the bear-off
    for ply in range(20):
        black = np_(env.get_state()["player"]) == -1
        obs, reward, term, trunc, info, aft, values, actions = player.step()
        o, v, codes = np_(aft.offsets), np_(values), np_(aft.codes)
        assert v.shape == (aft.cap,) and int(o[-1]) == aft.cap
        want = _pick_ref(o, aft.cap, v, black, "white")
        assert np.array_equal(np_(info["row"]), want), ply
        has = want >= 0
        assert np.array_equal(np_(actions)[has], codes[want[has]])  # a row of this ply's afterstates
        assert not np_(actions)[~has].any()
        assert np.array_equal(np_(info["actions"]), np_(actions))
        # a terminal row carries its outcome, and a winning one is played
        rew = np_(aft.reward)
        if (rew != 0).any():
            r = np.nonzero(rew != 0)[0]
            sign = np.where(black[np_(aft.row_env)[r]], -1.0, 1.0)
            assert np.array_equal(v[r], sign * rew[r])
        assert np.array_equal(np_(term)[has] != 0, rew[want[has]] != 0)
    env.close()


def test_full4_is_refused():
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device="cuda:0", rules="full4")
    with pytest.raises(ValueError):
        env.afterstates()
    env.close()
