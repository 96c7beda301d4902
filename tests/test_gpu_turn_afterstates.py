"""FULL4 whole-turn afterstates and value-greedy play on the GPU
(k_turn_count, k_turn_fill, k_turn_overflow, k_aft_scan, k_turn_pick through
VecNardeEnv.turn_afterstates / pick_turn and gym_narde.value_play.ValuePlayer),
every output bit for bit against the enumerator over oracle.full4_turn
(tests/turn_afterstates_ref.py), and against narde_step_full itself.
"""
import numpy as np
import pytest

import oracle as O
import turn_afterstates_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from afterstate_checks import _check_pick, _equal, _pick_ref, _scored_ply, np_  # noqa: E402
from afterstate_checks import _env as _env_of  # noqa: E402
B = 1003
BIG_AT = (0, 500, B - 1)  # the 2,065-row position: first env, mid-wave among light envs, last env
KEYS = ("board", "off", "ft", "player", "dice")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def case():
    """1,003 states -- the edge states, the start position under all 36 dice,
    self-play states, the 2,065-row position three times -- and their
    reference rows, computed once and left alone."""
    sp = R.selfplay_states()
    parts = [R.edge_states(), R.start_states()]
    n = B - sum(len(p["player"]) for p in parts)
    # every 2nd self-play state: all phases of the game
    parts.append({k: sp[k][::2][:n] for k in KEYS})
    st = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in KEYS}
    big = R.big_state()
    for e in BIG_AT:
        for k in KEYS:
            st[k][e] = big[k]
    assert len(st["player"]) == B
    ref = R.enumerate_turns(*(st[k] for k in KEYS))
    cnt = np.diff(ref["offsets"])
    assert all(cnt[e] == R.BIG_ROWS for e in BIG_AT) and (cnt == 0).any()
    # rows past the fast path's 256 nodes a level on some envs, not on most
    assert (cnt > 256).sum() == 3 and np.median(cnt) < 32
    return st, ref


def _env(st):
    return _env_of([st[k] for k in KEYS], rules="full4")


def test_rows_equal_the_enumerator(case):
    st, want = case
    env = _env(st)
    aft = env.turn_afterstates(dice=st["dice"], obs=True)
    assert aft.cap == int(want["offsets"][-1]) and aft.feat.shape == (aft.cap, 198)
    _equal(aft, want, action="play")
    # feat=False / obs=False leave those arrays out, the rest unchanged
    lean = env.turn_afterstates(dice=st["dice"], feat=False)
    assert lean.feat is None and lean.obs is None
    assert np.array_equal(np_(lean.play), want["play"]) and np.array_equal(np_(lean.offsets), want["offsets"])
    env.close()


def test_two_calls_give_identical_results(case):
    st, want = case
    env = _env(st)
    a = env.turn_afterstates(dice=st["dice"], obs=True)
    b = env.turn_afterstates(dice=st["dice"], obs=True)
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
    env.close()


def test_cap_cuts_rows_not_offsets_and_count_only(case):
    from gym_narde.vector import TurnAfterstates

    st, want = case
    env = _env(st)
    total = int(want["offsets"][-1])
    o = want["offsets"]
    # a cut inside the mid-wave heavy env's rows, at an odd row (a feature row
    # is 792 B: the run then ends 8 B into a 16-B piece)
    e = BIG_AT[1]
    cap = int(o[e]) + 700 + (int(o[e]) % 2 == 0)
    assert cap % 2 == 1 and o[e] < cap < o[e + 1] and cap < total
    dev = env.device
    out = TurnAfterstates(torch.zeros(B + 1, dtype=torch.int32, device=dev),
                          torch.full((total,), -7, dtype=torch.int32, device=dev),
                          torch.full((total, 4, 2), -7, dtype=torch.int8, device=dev),
                          torch.full((total, 198), -7.0, dtype=torch.float32, device=dev),
                          torch.full((total, 24), -7, dtype=torch.int32, device=dev),
                          torch.full((total,), -7, dtype=torch.int8, device=dev), cap)
    aft = env.turn_afterstates(dice=st["dice"], out=out)
    assert aft.cap == cap
    _equal(aft, want, rows=cap, action="play")  # offsets: the true counts
    assert int(np_(aft.offsets)[-1]) == total > cap
    for a in (aft.row_env, aft.play, aft.feat, aft.obs, aft.reward):
        assert (np_(a)[cap:] == -7).all()
    # count only: cap 0, no row array
    cnt = env.turn_afterstates(dice=st["dice"], cap=0)
    assert cnt.cap == 0 and np.array_equal(np_(cnt.offsets), want["offsets"])
    # pick ignores the cut rows: the best value sits in them
    values = torch.zeros(total, dtype=torch.float32, device=dev)
    values[cap:] = 9.0
    play, row = env.pick_turn(aft, values, perspective="mover")
    rows = np_(row)
    assert rows.max() < cap and rows[e] == o[e] and (rows[e + 1:] == -1).all()
    assert (np_(play)[e + 1:] == -1).all()
    env.close()


def test_device_dice_equal_given_dice():
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(B, device="cuda:0", seed=77, rules="full4")
    env.selfplay(37)
    a = env.turn_afterstates(obs=True)
    b = env.turn_afterstates(dice=env.dice(), obs=True)
    assert a.cap == b.cap and a.cap > B
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    s = env.get_state()
    want = R.enumerate_turns(np_(s["board"]), np_(s["off"]), np_(s["first_turn"]), np_(s["player"]), np_(env.dice()))
    _equal(a, want, action="play")
    env.close()


def test_ref2_is_refused():
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(8, device="cuda:0")
    with pytest.raises(ValueError):
        env.turn_afterstates()
    env.close()


@pytest.mark.parametrize("perspective", ["white", "mover"])
def test_pick_equals_torch_segments(case, perspective):
    st, want = case
    env = _env(st)
    aft = env.turn_afterstates(dice=st["dice"])
    rng = np.random.default_rng(9)
    v = rng.integers(0, 4, aft.cap).astype(np.float32) / 4 - 0.5  # four levels: ties everywhere
    v[rng.random(aft.cap) < 0.01] = np.nan
    black = st["player"] == -1
    assert black.any() and (~black).any()
    values = torch.from_numpy(v).to(env.device)
    rows = _check_pick(env, aft, values, black, perspective, want["play"])
    assert (rows == -1).sum() == (np.diff(want["offsets"]) == 0).sum()
    # a strided (R, 1) column of a wider tensor
    wide = torch.zeros((aft.cap, 3), dtype=torch.float32, device=env.device)
    wide[:, 1] = values
    _, r2 = env.pick_turn(aft, wide[:, 1:2], perspective=perspective)
    assert np.array_equal(np_(r2), rows)
    # epsilon 0: the same greedy rows
    _check_pick(env, aft, values, black, perspective, want["play"], epsilon=0.0, tag=5, seed=11)
    env.close()


@pytest.mark.parametrize("eps", [1.0, 0.3])
def test_pick_explore_draw(case, eps):
    st, want = case
    env = _env(st)
    aft = env.turn_afterstates(dice=st["dice"])
    rng = np.random.default_rng(2)
    v = rng.random(aft.cap).astype(np.float32)
    values = torch.from_numpy(v).to(env.device)
    seed, tag = 0x1234567890, 41
    play, row = env.pick_turn(aft, values, perspective="mover", epsilon=eps, tag=tag, seed=seed)
    o = want["offsets"].astype(np.int64)
    greedy = _pick_ref(o, aft.cap, v, st["player"] == -1, "mover")
    q32 = int(float(np.float32(eps)) * 4294967296.0)
    exp = np.full(B, -1, np.int64)
    explored = 0
    for e in range(B):
        cnt = int(o[e + 1] - o[e])
        if cnt:
            r = O.philox((tag, e, 0, 5), (seed & 0xFFFFFFFF, seed >> 32))
            if r[0] < q32:
                exp[e] = o[e] + ((r[1] * cnt) >> 32)
                explored += 1
            else:
                exp[e] = greedy[e]
    assert explored > 0 and (eps == 1.0 or explored < (exp >= 0).sum())
    assert np.array_equal(np_(row), exp)
    assert np.array_equal(np_(play), np.where((exp >= 0)[:, None, None], want["play"][np.maximum(exp, 0)], -1))
    env.close()


def test_step_carries_out_the_picked_play(case):
    """The picked plays, stepped: get_state() is the picked rows' position,
    the step's obs, reward and terminated are the rows'."""
    st, want = case
    env = _env(st)
    aft = env.turn_afterstates(dice=st["dice"], obs=True)
    rng = np.random.default_rng(5)
    values = torch.from_numpy(rng.random(aft.cap).astype(np.float32)).to(env.device)
    play, row = env.pick_turn(aft, values, perspective="white")
    obs, reward, term, _, info = env.step(play, st["dice"])
    feat = np_(env.tesauro198())
    s = env.get_state()
    r = np_(row).astype(np.int64)
    has = r >= 0
    r = r[has]
    assert has.sum() > 900 and (want["reward"][r] != 0).any()
    assert np.array_equal(np_(s["board"])[has], want["board"][r])
    assert np.array_equal(np_(s["off"])[has], want["off"][r])
    assert np.array_equal(np_(s["player"])[has], want["player"][r])
    assert np.array_equal(feat[has].view(np.uint32), want["feat"][r].view(np.uint32))
    assert np.array_equal(np_(obs)[has], want["obs"][r])
    assert np.array_equal(np_(reward)[has], want["reward"][r].astype(np.int32))
    assert np.array_equal(np_(term)[has] != 0, want["reward"][r] != 0)
    # an env with no row passes: its position stays, the mover changes
    assert np.array_equal(np_(s["board"])[~has], st["board"][~has])
    env.close()


def test_graph_capture_equals_eager():
    """turn_afterstates(cap) + a small MLP + pick_turn + step captured once and
    replayed five times: no allocation or synchronise inside the calls."""
    from gym_narde.vector import TurnAfterstates, VecNardeEnv

    n, cap, seed = 257, 257 * 96, 99
    envs = [VecNardeEnv(n, device="cuda:0", seed=seed, rules="full4") for _ in range(2)]
    dev = envs[0].device
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(198, 16), torch.nn.Sigmoid(), torch.nn.Linear(16, 1)).to(dev)
    score = lambda feat: net(feat).reshape(-1)  # noqa: E731
    mk = lambda: TurnAfterstates(torch.zeros(n + 1, dtype=torch.int32, device=dev),  # noqa: E731
                                 torch.zeros(cap, dtype=torch.int32, device=dev),
                                 torch.zeros((cap, 4, 2), dtype=torch.int8, device=dev),
                                 torch.zeros((cap, 198), dtype=torch.float32, device=dev), None,
                                 torch.zeros(cap, dtype=torch.int8, device=dev), cap)
    for e in envs:
        e.selfplay(25)
        e.turn_afterstates(cap=0)  # the handle's workspace, made outside capture
    outs = [mk(), mk()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.no_grad():
            net(outs[0].feat)  # the GEMM's own set-up, outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            g_play, g_row = _scored_ply(envs[0], outs[0], score)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        e_play, e_row = _scored_ply(envs[1], outs[1], score)
        torch.cuda.synchronize()
        assert 0 < int(outs[1].offsets[n]) <= cap
        assert torch.equal(g_play, e_play) and torch.equal(g_row, e_row)
        assert torch.equal(outs[0].offsets, outs[1].offsets)
    a, b = envs[0].get_state(), envs[1].get_state()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for e in envs:
        e.close()


def _words_of(board, off, ft, player, dice, play):
    """The pick words under which oracle.full4_turn makes `play` (n,4,2), and
    whether every sub-move is an entry of its C_k."""
    n = len(player)
    words = np.zeros((n, 4), np.uint32)
    ok = np.ones(n, bool)
    dh = dice.max(1).astype(np.int64)
    pos = np.arange(24, dtype=np.uint32)
    for k in range(4):
        r = O.full4_turn(board, off, ft, player, dice, words)
        f, d = play[:, k, 0].astype(np.int64), play[:, k, 1].astype(np.int64)
        on = f >= 0
        ok &= on == (r["max_dice"] > k)
        bits = ((r["cmask"][:, k, :, None] >> pos) & np.uint32(1)).astype(np.int64)  # (n, 2, 24)
        nc = bits.sum((1, 2))
        col = np.where(d == dh, 0, 1)
        fq = np.clip(f, 0, 23)
        idx = np.where(col == 1, bits[:, 0].sum(1), 0) + (bits[np.arange(n), col] * (pos[None, :] < fq[:, None])).sum(1)
        ok &= ~on | (bits[np.arange(n), col, fq] == 1)
        ncs = np.maximum(nc, 1)
        w = ((idx.astype(np.uint64) << np.uint64(32)) + (ncs - 1).astype(np.uint64)) // ncs.astype(np.uint64)
        words[:, k] = np.where(on & (nc > 0), w, 0).astype(np.uint32)
    return words, ok


def test_value_player_plays_whole_turns():
    """30 plies of a 4,099-env FULL4 handle under ValuePlayer: every ply's
    pick is the argmax of its own values, and the turn the env carries out is
    oracle.full4_turn's on the chosen play."""
    from gym_narde.value_play import ValuePlayer
    from gym_narde.vector import VecNardeEnv

    n = 4099
    env = VecNardeEnv(n, device="cuda:0", seed=2026, rules="full4", autoreset=False)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(198, 80), torch.nn.Sigmoid(), torch.nn.Linear(80, 1),
                              torch.nn.Sigmoid()).to(env.device)
    player = ValuePlayer(env, net, perspective="white")
    env.selfplay(75)  # random games end at plies 78..112: the 30 plies run through the bear-off
    terminal_rows = 0
    for ply in range(30):
        s0 = {k: np_(v) for k, v in env.get_state().items()}
        black = s0["player"] == -1
        obs, reward, term, trunc, info, aft, values, play = player.step()
        o, v, plays = np_(aft.offsets), np_(values), np_(aft.play)
        assert v.shape == (aft.cap,) and int(o[-1]) == aft.cap
        want = _pick_ref(o, aft.cap, v, black, "white")
        assert np.array_equal(np_(info["row"]), want), ply
        has = want >= 0
        pl = np_(play)
        assert np.array_equal(pl[has], plays[want[has]]) and (pl[~has] == -1).all()
        # a terminal row carries its outcome
        rew = np_(aft.reward)
        r = np.nonzero(rew != 0)[0]
        terminal_rows += len(r)
        sign = np.where(black[np_(aft.row_env)[r]], -1.0, 1.0)
        assert np.array_equal(v[r], sign * rew[r])
        # the oracle's turn on the chosen play
        dice = np_(info["dice"])
        words, ok = _words_of(s0["board"], s0["off"], s0["first_turn"], s0["player"], dice, pl)
        assert ok.all(), ply
        t = O.full4_turn(s0["board"], s0["off"], s0["first_turn"], s0["player"], dice, words)
        assert np.array_equal(t["played"], pl)
        assert np.array_equal(has, t["max_dice"] > 0)
        s1 = {k: np_(x) for k, x in env.get_state().items()}
        assert np.array_equal(s1["board"], t["board"]) and np.array_equal(s1["off"], t["off"])
        assert np.array_equal(np_(reward), t["reward"].astype(np.int32))
        assert np.array_equal(np_(term) != 0, t["done"] != 0)
    assert terminal_rows > 0
    env.close()
