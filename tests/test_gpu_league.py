"""The league launches on the GPU (k_value_rollout_league and
k_turn_value_rollout_league through VecNardeEnv.value_rollout_league /
turn_value_rollout_league, value_play.play_league and the C calls; DESIGN.md
section 27): a net per env and colour from a table.

The reference is the two-net call (value_rollout / turn_value_rollout with
records), which tests/test_gpu_value_rollout.py and
tests/test_gpu_turn_value_rollout.py pin to the composed per-ply calls: for
every distinct pair (i, j) of a launch a fresh env with the same seed, ids and
start state runs it under (nets[i], nets[j]) -- None for the random index; a
loop of random step() calls stands in for (-1, -1), which the two-net call
refuses -- and the envs of that pair must give the same bytes: every output
column (value as bytes, so NaNs count), the records, get_state(), stats() and
the ply counter.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from test_value_cpu import make_net
from test_value_rollout_cpu import endgames
from turn_afterstates_ref import BIG_ROWS, big_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, ENV0, PICK_SEED, TAG = 20251020, 3, 91, 500
SPECS = ((80, "sigmoid", "sigmoid", 1), (1, "tanh", "none", 3), (17, "tanh", "none", 6), (128, "sigmoid", "sigmoid", 2))
WHO = (0, 1, 2, 3, -1)
PAIRS25 = [(w, b) for w in WHO for b in WHO]  # (i, i) and (-1, -1) among them
RULES = ("ref2", "full4")
INT32_MIN = -(2 ** 31)
BIG_SEED = 20251022  # envs 2, 24, 29 and 34 of 64 roll 1-1 first


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def nets():
    return [make_net(*s).to("cuda:0") for s in SPECS]


def np_(x):
    return x.detach().cpu().numpy()


def make_env(B, max_steps=1000, state=None, rules="ref2", seed=SEED):
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(B, device="cuda:0", seed=seed, env_id_offset=ENV0, max_episode_steps=max_steps, rules=rules)
    if state is not None:
        env.set_state(*(torch.as_tensor(a).to(env.device) for a in state))
    return env


def i32(x, device="cuda:0"):
    return torch.as_tensor(np.asarray(x, dtype=np.int64).astype(np.int32), device=device)


def cycle(pairs, B):
    w = [pairs[e % len(pairs)][0] for e in range(B)]
    b = [pairs[e % len(pairs)][1] for e in range(B)]
    return w, b


def launch(env, plies, table, white, black, **kw):
    """The rule set's league launch with every output and the records."""
    if env.full:
        bufs = env.turn_value_rollout_buffers(plies, records=True)
        return env.turn_value_rollout_league(plies, table, white, black, bufs=bufs, **kw)
    bufs = env.value_rollout_buffers(plies, records=True)
    return env.value_rollout_league(plies, table, white, black, bufs=bufs, **kw)


def two_net(env, plies, net_w, net_b, **kw):
    if env.full:
        bufs = env.turn_value_rollout_buffers(plies, records=True)
        return env.turn_value_rollout(plies, net_w, net_b, bufs=bufs, **kw)
    return env.value_rollout(plies, net_w, net_b, bufs=env.value_rollout_buffers(plies, records=True), **kw)


def random_loop(env, plies):
    """(-1, -1): plies random step() calls, as the columns of a launch (no
    records: step() has no such output)."""
    col = "play" if env.full else "actions"
    out = {k: [] for k in ("dice", col, "value", "reward", "terminated", "truncated")}
    for _ in range(plies):
        out["dice"].append(np_(env.dice()).copy())
        _, rew, term, trunc, info = env.step()
        if env.full:
            out[col].append(np_(info["played"]).copy().view(np.int8).reshape(-1, 4, 2))
        else:
            out[col].append(np_(info["actions"]).copy())
        out["value"].append(np.full(env.num_envs, np.nan, np.float32))
        out["reward"].append(np_(rew).copy())
        out["terminated"].append(np_(term).copy())
        out["truncated"].append(np_(trunc).copy())
    return {k: np.stack(v) for k, v in out.items()}


def snapshot(env):
    st = {k: np_(v) for k, v in env.get_state().items()}
    return st, np_(env.stats()), int(env.ply)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same_launch(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert same_bytes(np_(a[k]), np_(b[k])), f"{what}: {k}"


def assert_same_env(a, b):
    (sa, ta, pa), (sb, tb, pb) = snapshot(a), snapshot(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(ta, tb) and pa == pb


def norm(i, n):
    return i if 0 <= i < n else -1


def check_against_two_net(rules, B, plies, nets, white, black, got, env, max_steps=1000, state=None, what="",
                          env_seed=SEED, **kw):
    """Every env of `env` (after the league launch that gave `got`) against
    the two-net reference of its pair.  Returns {pair: compared plies}."""
    n = len(nets)
    got = {k: np_(v) for k, v in got.items()}
    gst, gstats, gply = snapshot(env)
    pairs = {}
    for e in range(B):
        pairs.setdefault((norm(white[e], n), norm(black[e], n)), []).append(e)
    counts = {}
    for (i, j), envs in sorted(pairs.items()):
        ref = make_env(B, max_steps, state, rules, env_seed)
        if i < 0 and j < 0:
            want = random_loop(ref, plies)
        else:
            want = {k: np_(v) for k, v in two_net(ref, plies, nets[i] if i >= 0 else None,
                                                  nets[j] if j >= 0 else None, **kw).items()}
        rst, rstats, rply = snapshot(ref)
        ref.close()
        assert rply == gply, f"{what} pair {(i, j)}: ply counter"
        for e in envs:
            for k, w in want.items():
                assert same_bytes(got[k][:plies, e], w[:plies, e]), f"{what} pair {(i, j)} env {e}: {k}"
            for k in gst:
                assert np.array_equal(gst[k][e], rst[k][e]), f"{what} pair {(i, j)} env {e}: state {k}"
            assert np.array_equal(gstats[e], rstats[e]), f"{what} pair {(i, j)} env {e}: stats"
        counts[(i, j)] = plies * len(envs)
    print(f"{what}: compared plies per pair {counts}")
    return counts


def run_case(rules, B, plies, nets, pairs=PAIRS25, max_steps=1000, state=None, scratch_pieces=None, what="",
             env_seed=SEED, **kw):
    env = make_env(B, max_steps, state, rules, env_seed)
    table = env.net_table(nets)
    white, black = cycle(pairs, B)
    extra = dict(kw)
    if scratch_pieces is not None:
        extra["scratch"] = env.turn_value_rollout_scratch(scratch_pieces)
    got = launch(env, plies, table, i32(white), i32(black), **extra)
    counts = check_against_two_net(rules, B, plies, nets, white, black, got, env, max_steps, state, what, env_seed, **kw)
    return env, got, counts


def test_per_env_equality_ref2(nets):
    env, _, counts = run_case("ref2", 65, 7, nets, what="ref2 B 65")
    assert len(counts) == 25 and min(counts.values()) >= 2 * 7  # every pair has at least 2 envs
    assert env.ply == 7
    env.close()


def test_per_env_equality_full4(nets):
    env, got, counts = run_case("full4", 65, 7, nets, what="full4 B 65, default scratch")
    assert len(counts) == 25 and min(counts.values()) >= 2 * 7
    # a piece an env: the same bits
    big = make_env(65, rules="full4")
    white, black = cycle(PAIRS25, 65)
    again = launch(big, 7, big.net_table(nets), i32(white), i32(black), scratch=big.turn_value_rollout_scratch(65))
    assert_same_launch(got, again, "65 pieces")
    assert_same_env(env, big)
    env.close()
    big.close()
    # 7 envs on 3 waves: the waves play 3, 2 and 2 envs with different pairs one after another
    pairs7 = [(0, 1), (-1, 3), (2, 2), (3, -1), (1, 0), (-1, -1), (2, 3)]
    small, got3, counts = run_case("full4", 7, 7, nets, pairs=pairs7, scratch_pieces=3, what="full4 B 7, 3 pieces")
    assert len(counts) == 7
    whole = make_env(7, rules="full4")
    white, black = cycle(pairs7, 7)
    got7 = launch(whole, 7, whole.net_table(nets), i32(white), i32(black), scratch=whole.turn_value_rollout_scratch(7))
    assert_same_launch(got3, got7, "3 pieces against 7")
    assert_same_env(small, whole)
    small.close()
    whole.close()


def test_full4_a_level_past_the_chip_tier_walks_in_the_slab(nets):
    """big_state() (2,065 rows under 1-1: a level past the 256-node tier, so
    the walk runs again in the wave's slab piece) on exactly the envs of a
    B = 64 batch whose first roll is 1-1 (BIG_SEED: SEED's first rolls have no
    1-1 among 64 envs); white, big_state()'s mover, has a net in every pair; 3
    pieces of scratch, so an overflowing env shares its wave's piece with the
    envs before and behind it."""
    B, plies = 64, 2
    pairs = [(0, 1), (1, -1), (2, 3), (3, 0)]
    probe = make_env(B, rules="full4", seed=BIG_SEED)
    first = np_(probe.dice())
    base = {k: np_(v) for k, v in probe.get_state().items()}
    ones = np.flatnonzero((first == 1).all(1))
    assert len(ones) >= 1, "no env of the batch rolls 1-1 first: choose another seed"
    big = big_state()
    assert big["player"] == 1
    board, off, ft, player = (base[k].copy() for k in ("board", "off", "first_turn", "player"))
    board[ones], off[ones], ft[ones], player[ones] = big["board"], big["off"], big["ft"], big["player"]
    probe.set_state(*(torch.as_tensor(a).to(probe.device) for a in (board, off, ft, player)))
    rows = np.diff(np_(probe.turn_afterstates(feat=False).offsets))
    assert (rows[ones] == BIG_ROWS).all() and rows.max() == BIG_ROWS
    probe.close()
    env, _, counts = run_case("full4", B, plies, nets, pairs=pairs, state=(board, off, ft, player), scratch_pieces=3,
                              what="full4 big_state on the 1-1 envs", env_seed=BIG_SEED)
    assert len(counts) == 4
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_index_rule(rules, nets):
    """n_nets, 32,767, -2 and INT32_MIN are index -1; nothing behind the
    table's last entry is read or written."""
    B, plies, n = 65, 7, 3
    entry = 64
    slab = torch.full((entry * n + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")  # sentinels behind the table
    outside = (n, 32767, -2, INT32_MIN)
    inside = (0, 1, 2)
    white = [outside[e % 4] if e % 3 else inside[e % 3] for e in range(B)]
    black = [outside[(e // 2) % 4] if e % 2 else inside[e % 3] for e in range(B)]
    assert any(w in outside and b in outside for w, b in zip(white, black))
    a, b = make_env(B, rules=rules), make_env(B, rules=rules)
    table = a.net_table(nets[:n], out=slab)
    assert table.numel() == entry * n and table.data_ptr() == slab.data_ptr()
    got = launch(a, plies, table, i32(white), i32(black))
    want = launch(b, plies, table, i32([norm(x, n) for x in white]), i32([norm(x, n) for x in black]))
    assert_same_launch(got, want, "outside indices against -1")
    assert_same_env(a, b)
    assert bool((slab[entry * n:] == 0xA5).all()), "written behind the table"
    # (a read of entry n would have taken a net of 0xA5 bytes: index n plays the random policy's bits above,
    # and the whole launch equals the two-net references, where no such entry exists)
    check_against_two_net(rules, B, plies, nets[:n], white, black, got, a, what=f"{rules} index rule")
    a.close()
    b.close()


@pytest.mark.parametrize("rules", RULES)
def test_explore_draws(rules, nets):
    env, got, counts = run_case(rules, 65, 7, nets, what=f"{rules} epsilon 0.3", epsilon=0.3, tag=TAG, seed=PICK_SEED)
    greedy = make_env(65, rules=rules)
    white, black = cycle(PAIRS25, 65)
    plain = launch(greedy, 7, greedy.net_table(nets), i32(white), i32(black))
    col = "play" if rules == "full4" else "actions"
    assert not same_bytes(np_(got[col]), np_(plain[col])), "no explore ply changed a play"
    env.close()
    greedy.close()


@pytest.mark.parametrize("rules", RULES)
def test_truncation_and_resets_inside_a_launch(rules, nets):
    B = 65
    env, got, _ = run_case(rules, B, 7, nets, max_steps=5, what=f"{rules} max_episode_steps 5")
    resets = int((np_(got["terminated"]) | np_(got["truncated"])).sum())
    assert resets >= B and int(np_(got["truncated"]).sum()) >= B
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_terminal_rows_are_picked_and_the_pair_plays_the_next_game(rules, nets):
    B = 65
    state = tuple(np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:])) for a in endgames())
    env, got, _ = run_case(rules, B, 5, nets, state=state, what=f"{rules} endgames")
    term = np_(got["terminated"])
    assert term[0].all(), "one ply from winning: ply 0 ends every env's game"
    rew = np_(got["reward"])[0]
    assert set(np.unique(rew).tolist()) == {1, 2}
    value = np_(got["value"])
    white, black = cycle(PAIRS25, B)
    mover0 = np.where(state[3] == 1, np.asarray(white), np.asarray(black))
    # a net's ply 0 picked the terminal row at its outcome (white's value); a random mover's value is NaN
    sign = np.where(state[3] == 1, 1.0, -1.0)
    has = mover0 >= 0
    assert np.array_equal(value[0][has], (sign * rew)[has].astype(np.float32)) and np.isnan(value[0][~has]).all()
    # plies 1 ..: the next game, under the same pair (the references' bits above); an env of two nets has values
    # there, an env of none has not
    both = (np.asarray(white) >= 0) & (np.asarray(black) >= 0)
    neither = (np.asarray(white) < 0) & (np.asarray(black) < 0)
    assert (~np.isnan(value[1:, both])).any() and np.isnan(value[:, neither]).all()
    assert int(np_(env.stats())[:, 0].sum()) >= B
    env.close()


def test_padded_stride(nets):
    """One entry with ld_w1t = H + 4 and 1e9 in the padding: the packed net's bits."""
    from gym_narde import _lib

    B, plies = 65, 7
    env, ref = make_env(B), make_env(B)
    white, black = cycle(PAIRS25, B)
    want = launch(ref, plies, ref.net_table(nets), i32(white), i32(black))
    structs = (_lib.ValueMlp * 4)(*[g.struct() for g in nets])
    g = nets[2]
    H = g.hidden
    w1t = torch.full((198, H + 4), 1e9, dtype=torch.float32, device=env.device)  # a read past H would show
    w1t[:, :H] = g.l1.weight.detach().t()
    structs[2].w1t, structs[2].ld_w1t = w1t.data_ptr(), H + 4
    table = torch.empty(_lib.league_table_bytes(4), dtype=torch.uint8, device=env.device)
    _lib.check(env.handle.lib.narde_net_table(0, 4, structs, _lib.ptr(table), table.numel(), env._s()),
               "narde_net_table")
    got = launch(env, plies, table, i32(white), i32(black))
    assert_same_launch(got, want, "padded stride")
    assert_same_env(env, ref)
    env.close()
    ref.close()


@pytest.mark.parametrize("rules", RULES)
def test_loop_carry_and_determinism(rules, nets):
    """One 7-ply launch = seven 1-ply launches with tag + k = the same
    launch on a fresh env."""
    B, plies = 65, 7
    a, b, c = (make_env(B, 5, rules=rules) for _ in range(3))
    white, black = (i32(x) for x in cycle(PAIRS25, B))
    kw = dict(epsilon=0.3, seed=PICK_SEED)
    table = a.net_table(nets)
    one = {k: v.clone() for k, v in launch(a, plies, table, white, black, tag=TAG, **kw).items()}
    again = launch(c, plies, table, white, black, tag=TAG, **kw)
    assert_same_launch(one, again, "a fresh env")
    steps = [{k: np_(v) for k, v in launch(b, 1, table, white, black, tag=TAG + k, **kw).items()} for k in range(plies)]
    for k in one:
        assert same_bytes(np_(one[k]), np.concatenate([s[k] for s in steps])), k
    assert_same_env(a, b)
    assert_same_env(a, c)
    assert a.ply == plies
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("rules", RULES)
def test_graph_replay(rules):
    """A captured 3-ply launch, replayed twice with white, black and the
    weights rewritten in place in between, against an eager env."""
    B = 65
    own = [make_net(*s).to("cuda:0") for s in SPECS]  # (their weights change here)
    for g in own:
        g.pack()
    a, b = make_env(B, rules=rules), make_env(B, rules=rules)
    table = a.net_table(own)
    w0, b0 = cycle(PAIRS25, B)
    w1, b1 = cycle(PAIRS25[7:] + PAIRS25[:7], B)
    white, black = i32(w0), i32(b0)
    make = a.turn_value_rollout_buffers if a.full else a.value_rollout_buffers
    bufs = make(3, records=True)
    call = a.turn_value_rollout_league if a.full else a.value_rollout_league
    call(3, table, white, black, bufs=bufs)  # outside capture: plies 0..2 (and the FULL4 scratch)
    launch(b, 3, table, white, black)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call(3, table, white, black, bufs=bufs)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()  # plies 3..5
    torch.cuda.synchronize()
    assert_same_launch(bufs, launch(b, 3, table, white, black), "window 1")
    assert_same_env(a, b)
    white.copy_(i32(w1))
    black.copy_(i32(b1))
    with torch.no_grad():
        for g in own:
            g.l1.weight.mul_(-0.5)
            g.l2.bias.add_(0.25)
            g.pack()
    before = {k: v.clone() for k, v in bufs.items()}
    graph.replay()  # plies 6..8: other pairs, other weights
    torch.cuda.synchronize()
    assert_same_launch(bufs, launch(b, 3, table, white, black), "window 2")
    assert_same_env(a, b)
    col = "play" if a.full else "actions"
    assert not same_bytes(np_(before[col]), np_(bufs[col]))
    a.close()
    b.close()


def test_table_build_inside_a_graph(nets):
    env = make_env(4)
    want = env.net_table(nets).clone()
    assert want.dtype == torch.uint8 and want.numel() == 64 * len(nets) and bool((want != 0).any())
    out = torch.zeros(64 * len(nets), dtype=torch.uint8, device=env.device)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            env.net_table(nets, out=out)
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # 64 nets: four launches of 16
    many = [nets[i % 4] for i in range(64)]
    full = env.net_table(many)
    torch.cuda.synchronize()
    assert torch.equal(full.view(64, 64), want.view(4, 64).repeat(16, 1))
    env.close()


# the smallest ply count, in steps of 10, at which every pairing of test_play_league_end_to_end's launch had
# finished a game (measured on an MI355X; at 100 / 80 plies a pairing still had none); the tests run twice that
LEAGUE_PLIES_MIN = {"ref2": 110, "full4": 90}


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rules", RULES)
def test_play_league_end_to_end(rules, nets):
    from gym_narde.value_play import play_league

    env = make_env(256, rules=rules)
    res = play_league(env, nets[:2], 2 * LEAGUE_PLIES_MIN[rules], random=True, seed=PICK_SEED)
    assert res["pairs"] == [(0, 1), (0, -1), (1, 0), (1, -1), (-1, 0), (-1, 1)]
    g = res["games"]
    assert g.shape == (3, 3) and all(g[i][j] > 0 for i in range(3) for j in range(3) if i != j), g
    assert (np.diag(g) == 0).all()
    totals = [int(res[k].sum()) for k in ("games", "points_white", "points_black")]
    assert totals == np_(env.stats()).sum(0).tolist()
    m = res["margin"]
    assert np.array_equal(m[~np.eye(3, dtype=bool)], -m.T[~np.eye(3, dtype=bool)]) and np.isnan(np.diag(m)).all()
    assert not np.isnan(res["score"]).any()
    env.close()


def test_league_example_on_two_saved_files(tmp_path, capsys):
    paths = []
    for i, spec in enumerate(((80, "sigmoid", "tanh", 11), (17, "sigmoid", "tanh", 12))):
        paths.append(str(tmp_path / f"agent{i}.pt"))
        torch.save(make_net(*spec).state_dict(), paths[-1])
    res = _example("league_value_agents").main(paths, random=True, envs=256, plies=2 * LEAGUE_PLIES_MIN["ref2"],
                                               seed=3, device="cuda:0")
    out = capsys.readouterr().out
    assert "margin" in out and "random play" in out and "agent0.pt" in out and "games a pairing" in out
    assert res["games"].shape == (3, 3) and int(res["games"].sum()) > 0


def test_python_errors(nets):
    env = make_env(8)
    table = env.net_table(nets)
    white, black = i32([0] * 8), i32([1] * 8)
    with pytest.raises(ValueError):
        env.turn_value_rollout_league(2, table, white, black)  # the wrong rule set
    with pytest.raises(ValueError):
        env.value_rollout_league(0, table, white, black)
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table, white, black, epsilon=0.1)
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table.cpu(), white, black)  # a table from another device
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table[:63], white, black)
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table, white[:7], black)  # the wrong shape
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table, white, black.long())  # the wrong dtype
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table, white.cpu(), black)
    with pytest.raises(ValueError):
        env.value_rollout_league(2, table, [0] * 8, black)
    with pytest.raises(ValueError):
        env.value_rollout_league(3, table, white, black, bufs=env.value_rollout_buffers(2))
    with pytest.raises(ValueError):
        env.net_table([])
    with pytest.raises(ValueError):
        env.net_table([nets[0]] * 65)
    with pytest.raises(TypeError):
        env.net_table([torch.nn.Linear(198, 1).to(env.device)])
    with pytest.raises(ValueError):
        env.net_table([make_net(*SPECS[1])])  # a net on the CPU
    with pytest.raises(ValueError):
        env.net_table(nets, out=torch.empty(64 * 4 - 1, dtype=torch.uint8, device=env.device))
    from gym_narde.value_play import play_league

    with pytest.raises(ValueError):
        play_league(env, nets, 2)  # 12 pairs, 8 envs
    with pytest.raises(ValueError):
        play_league(env, [nets[0]] * 65, 2)
    with pytest.raises(ValueError):
        play_league(env, [make_net(*SPECS[1])], 2)
    env.close()
    full = make_env(8, rules="full4")
    with pytest.raises(ValueError):
        full.value_rollout_league(2, table, white, black)
    with pytest.raises(ValueError):
        full.turn_value_rollout_league(2, table, white, black, scratch=torch.empty(16, dtype=torch.uint8,
                                                                                   device=full.device))
    full.close()
