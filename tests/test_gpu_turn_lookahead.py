"""The FULL4 two-ply lookahead on the GPU (the record fills, k_turn_look, its
overflow pass and the mean through VecNardeEnv.lookahead_turn_afterstates and
LookaheadPlayer): the structural outputs bit for bit
against scored_turn_afterstates(), the values against the float64 reference
pipeline of tests/turn_lookahead_ref.py within tol = 8 x E, E = max |pipeline
in torch float32 - in float64| on the same rows, floored at one float32 ulp
of the largest magnitude compared (tests/test_lookahead_cpu.py states the
argument); terminal rows exact.

The reference uses only calls that existed before the lookahead: a second
FULL4 env holding the rows' records (set_state to the rows' parents,
step(play, dice) with autoreset off), turn_afterstates(feat=True) and
scored_turn_afterstates() on it per roll, and for a pass the position the
step with an all -1 play leaves, its tesauro198() and the dense net.  The
replies of a state set are fetched once and shared by the tests that use it.
"""
import copy
import ctypes

import numpy as np
import pytest

import turn_afterstates_ref as R
from test_value_cpu import TOL_FACTOR, make_net

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import lookahead_ref as LR  # noqa: E402
import turn_lookahead_ref as TL  # noqa: E402
from afterstate_checks import _env as _env_of  # noqa: E402
from afterstate_checks import _pick_ref, np_  # noqa: E402

KEYS = ("board", "off", "ft", "player", "dice")
SIGMOID80 = (80, "sigmoid", "sigmoid", 1)
TANH17 = (17, "tanh", "none", 6)
NETS = [(1, "relu", "none", 3), TANH17, SIGMOID80, (128, "sigmoid", "sigmoid", 2)]
SPLIT_ROWS = 3072  # kTurnLookSplitRows: up to here a row's rolls go over four waves


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _env(st, **kw):
    return _env_of([st[k] for k in KEYS], rules="full4", **kw)


def _sub(st, idx):
    return {k: np.ascontiguousarray(np.asarray(st[k])[idx]) for k in KEYS}


@pytest.fixture(scope="module")
def states():
    """65 self-play states, 13 games at plies 0 (the start position: a
    first-turn replier), 20, 40, 60 and 80 -- a ply-40 state first."""
    sp = R.selfplay_states(n=13, plies=100, every=20, seed=11)
    assert len(sp["player"]) == 65
    return _sub(sp, np.roll(np.arange(65), -26))


def nets(spec, device):
    """The net on the device and its CPU twin (the reference)."""
    cpu = make_net(*spec)
    return copy.deepcopy(cpu).to(device), cpu


_REPLIES = {}


def row_replies(name, st, aft, dice_mode="all36"):
    """The rows' records on a second env, and per roll the live rows' replies
    (fetched once per `name`; None: not kept).  Returns a dict: live (R,)
    mask, rec (the live rows' board, off, first_turn, player tensors), black
    (live,) bool: black replies, ks, replies as lookahead_ref.two_ply takes
    them."""
    if name is not None and name in _REPLIES:
        return _REPLIES[name]
    dev = aft.row_env.device
    e = aft.row_env.long()
    parent = [torch.as_tensor(np.asarray(st[k])).to(dev)[e] for k in KEYS]
    rows = _env_of(parent[:4], rules="full4", dice_mode=dice_mode)
    rows.step(aft.play, parent[4])
    rec = rows.get_state()
    live = np_(aft.reward) == 0
    assert np.array_equal(np_(rows.terminated) != 0, ~live)
    idx = torch.from_numpy(np.nonzero(live)[0]).to(dev)
    rec = [rec[k][idx].clone() for k in ("board", "off", "first_turn", "player")]
    rows.close()
    n = len(idx)
    ks = TL.rolls_of(dice_mode)
    replies = []
    if n:
        lv = _env_of(rec, rules="full4", dice_mode=dice_mode)
        none = torch.full((n, 4, 2), -1, dtype=torch.int8, device=dev)
        for k in ks:
            d = torch.tensor([TL.ROLLS[k]], dtype=torch.uint8, device=dev).repeat(n, 1)
            lv.set_state(*rec)
            r = lv.turn_afterstates(dice=d)
            feat = np_(r.feat)
            rep = dict(offsets=np_(r.offsets), feat=feat, reward=np_(r.reward),
                       player=np.where(feat[:, 197] > 0.5, -1, 1).astype(np.int8))
            lv.step(none, d)  # a pass: what the step with an all -1 play leaves
            rep.update(pass_feat=np_(lv.tesauro198()), pass_reward=np_(lv.reward).astype(np.int8),
                       pass_player=np_(lv.get_state()["player"]))
            replies.append(rep)
        lv.close()
    c = dict(live=live, rec=rec, black=np_(rec[3]) == -1, ks=ks, replies=replies)
    if name is not None:
        _REPLIES[name] = c
    return c


def expected(cpu, c):
    """(fp64 values of the live rows, E)."""
    if not c["live"].any():
        return np.zeros(0), 0.0
    want, w32, _ = TL.two_ply_weighted(cpu, c["replies"], c["ks"], c["black"])
    return want, TL.error_bound(w32, want)


def composed(net, cpu, c):
    """The same valuation built from scored_turn_afterstates() per roll on an
    env of the rows' records, the pass from the dense net, the best by
    segment_best and the weighted mean in float64."""
    rec, n = c["rec"], len(c["black"])
    dev = rec[0].device
    lv = _env_of(rec, rules="full4")
    dense = copy.deepcopy(cpu).double()
    ms = []
    for k, rep in zip(c["ks"], c["replies"]):
        d = torch.tensor([TL.ROLLS[k]], dtype=torch.uint8, device=dev).repeat(n, 1)
        a, v = lv.scored_turn_afterstates(net, dice=d)
        assert np.array_equal(np_(a.offsets), rep["offsets"])
        with torch.no_grad():
            fb = LR.outcomes(dense(torch.from_numpy(rep["pass_feat"]).double()).reshape(-1), rep["pass_reward"],
                             rep["pass_player"])
        ms.append(LR.segment_best(v.cpu().double(), rep["offsets"], c["black"], fb))
    lv.close()
    w = torch.tensor([TL.WEIGHTS[k] for k in c["ks"]], dtype=torch.float64)
    return ((torch.stack(ms, 1) * w).sum(1) / w.sum()).numpy()


def check(values, want, E, live, what):
    """Live rows within 8 E."""
    got = np_(values) if torch.is_tensor(values) else values
    err = float(np.abs(got[live].astype(np.float64) - want).max()) if live.any() else 0.0
    print(f"{what}: E = {E:.3e}, max error = {err:.3e} = {err / max(E, 1e-30):.2f} E")
    assert err <= TOL_FACTOR * E, (what, err, TOL_FACTOR * E)
    return err


def terminal_outcomes(st, aft):
    """The terminal rows' outcomes: reward, negated when black made the move."""
    r = np_(aft.reward).astype(np.float32)
    mover = np.asarray(st["player"])[np_(aft.row_env)]
    return np.where(mover == -1, -r, r)


def same_rows(aft, one):
    for k in ("offsets", "row_env", "play", "reward"):
        assert torch.equal(getattr(aft, k), getattr(one, k)), k


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
@pytest.mark.parametrize("B", [1, 65])
def test_rows_and_values(states, B, spec):
    st = _sub(states, np.arange(B))
    env = _env(st)
    net, cpu = nets(spec, env.device)
    one, v1 = env.scored_turn_afterstates(net, dice=st["dice"])
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    assert aft.feat is None and aft.obs is None and aft.cap == one.cap and values.shape == (one.cap,)
    assert 0 < aft.cap <= SPLIT_ROWS
    same_rows(aft, one)
    c = row_replies(f"first{B}", st, aft)
    want, E = expected(cpu, c)
    live = c["live"]
    check(values, want, E, live, f"B={B} {spec[:3]}")
    assert np.array_equal(np_(values)[~live], terminal_outcomes(st, aft)[~live])
    # the composed form: the parent's scored calls per roll give the same values
    check(composed(net, cpu, c), want, E, np.ones(int(live.sum()), bool), f"B={B} {spec[:3]} composed")
    # not the one-ply values
    assert float((values - v1).abs().max()) > 1e3 * TOL_FACTOR * E
    # the same bits on a second call
    again = env.lookahead_turn_afterstates(net, dice=st["dice"])[1]
    assert torch.equal(values.view(torch.int32), again.view(torch.int32))
    env.close()


def test_many_workgroups_and_terminal_rows():
    """B = 257: workgroups beyond a handful, and states whose rows end the
    game for either colour (the edge states).  The other 245 are the
    self-play states with the fewest rows, which keeps the reference small."""
    sp = R.selfplay_states(n=32, plies=120, every=4, seed=7)
    probe = _env(sp)
    cnt = np.diff(np_(probe.turn_afterstates(dice=sp["dice"], cap=0).offsets))
    probe.close()
    few = np.nonzero((cnt >= 1) & (cnt <= 6))[0][:245]
    assert len(few) == 245
    st = R.concat(_sub(sp, few), R.edge_states())
    assert len(st["player"]) == 257
    env = _env(st)
    net, cpu = nets(SIGMOID80, env.device)
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    one, v1 = env.scored_turn_afterstates(net, dice=st["dice"])
    same_rows(aft, one)
    c = row_replies("b257", st, aft)
    want, E = expected(cpu, c)
    live = c["live"]
    out = terminal_outcomes(st, aft)
    assert (out[~live] > 0).any() and (out[~live] < 0).any()  # terminal rows of both colours
    check(values, want, E, live, "B=257")
    assert np.array_equal(np_(values)[~live], out[~live])
    assert torch.equal(values[torch.from_numpy(~live)], v1[torch.from_numpy(~live)])
    assert float((values - v1).abs().max()) > 1e3 * TOL_FACTOR * E
    again = env.lookahead_turn_afterstates(net, dice=st["dice"])[1]
    assert torch.equal(values.view(torch.int32), again.view(torch.int32))
    env.close()


def test_root_overflow_rows_are_valued(states):
    """big_state() as the root env beside an ordinary one, H = 17: its 2,065
    rows come through the overflow record fill and every one is valued."""
    big = R.big_states()
    st = R.concat(big, _sub(states, np.arange(1)))
    env = _env(st)
    net, cpu = nets(TANH17, env.device)
    one, v1 = env.scored_turn_afterstates(net, dice=st["dice"])
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    same_rows(aft, one)
    assert int(aft.offsets[1]) == R.BIG_ROWS and aft.cap > R.BIG_ROWS
    c = row_replies("root_overflow", st, aft)
    want, E = expected(cpu, c)
    assert c["live"].all()
    check(values, want, E, c["live"], "root overflow")
    assert float((values - v1).abs().max()) > 1e3 * TOL_FACTOR * E
    env.close()


def test_reply_overflow_tiers(states):
    """The two positions tests/test_turn_lookahead_cpu.py found: a row whose
    1-1 reply has a level above 2,048 nodes (the slab tier) and rows whose
    replies' largest levels lie in 257..2,048 (the LDS tier), valued within
    8 E; the ordinary env beside them, which takes no overflow path, gets the
    bits it gets alone."""
    third = _sub(states, np.arange(1))
    st = R.concat(TL.tier_state(TL.TIER_SLAB_POINTS), TL.tier_state(TL.TIER_LDS_POINTS), third)
    env = _env(st)
    net, cpu = nets(TANH17, env.device)
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    o = np_(aft.offsets)
    assert o[1] == 1 and o[2] == 5  # one row hands big_state() over; four rows of the LDS-tier parent
    c = row_replies("tiers", st, aft)
    cnt = np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1)
    assert cnt[0, 0] == R.BIG_ROWS and 256 < cnt[1:5].max() <= 2048 and cnt[5:].max() <= 256
    want, E = expected(cpu, c)
    check(values, want, E, c["live"], "reply overflow tiers")
    alone = _env(third)
    a1, v1 = alone.lookahead_turn_afterstates(net, dice=third["dice"])
    assert a1.cap == aft.cap - 5 and torch.equal(values[5:].view(torch.int32), v1.view(torch.int32))
    alone.close()
    env.close()


def test_padded_weight_rows(states):
    """ld_w1t = H + 4 through the C call: the bits of the dense layout."""
    from gym_narde import _lib

    st = states
    env = _env(st)
    dev = env.device
    for spec in (TANH17, SIGMOID80):
        net, _ = nets(spec, dev)
        aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
        H, cap = net.hidden, aft.cap
        wide = torch.full((198, H + 4), 1e9, dtype=torch.float32, device=dev)  # a read past H would show
        wide[:, :H] = net.l1.weight.detach().t()
        mlp = net.struct()
        mlp.w1t, mlp.ld_w1t = wide.data_ptr(), H + 4
        d = torch.as_tensor(st["dice"], dtype=torch.uint8, device=dev).contiguous()
        offsets = torch.zeros(66, dtype=torch.int32, device=dev)
        v = torch.zeros(cap, dtype=torch.float32, device=dev)
        scratch = torch.empty(_lib.turn_lookahead_scratch_bytes(cap), dtype=torch.uint8, device=dev)
        env.handle.call("narde_turn_afterstates_lookahead", _lib.ptr(d), cap, _lib.ptr(offsets), None, None, None,
                        ctypes.byref(mlp), 1, _lib.ptr(v), _lib.ptr(scratch), scratch.numel(), env._s())
        assert torch.equal(offsets, aft.offsets)
        assert torch.equal(v.view(torch.int32), values.view(torch.int32))
    env.close()


def _sentinel_out(dev, rows, cap):
    from gym_narde.vector import TurnAfterstates

    out = TurnAfterstates(torch.zeros(66, dtype=torch.int32, device=dev),
                          torch.full((rows,), -7, dtype=torch.int32, device=dev),
                          torch.full((rows, 4, 2), -7, dtype=torch.int8, device=dev), None, None,
                          torch.full((rows,), -7, dtype=torch.int8, device=dev), cap)
    return out, torch.full((rows,), -7.0, dtype=torch.float32, device=dev)


def test_cap_cuts_values_not_offsets(states):
    st = states
    env = _env(st)
    net, _ = nets(SIGMOID80, env.device)
    full, vfull = env.lookahead_turn_afterstates(net, dice=st["dice"])
    o = np_(full.offsets)
    total = int(o[-1])
    e = int(np.nonzero(np.diff(o) >= 5)[0][20])
    cap = int(o[e]) + 2
    assert o[e] < cap < o[e + 1] and cap < total
    out, vals = _sentinel_out(env.device, total, cap)
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"], out=(out, vals))
    assert aft.cap == cap and values.shape == (cap,)
    assert np.array_equal(np_(aft.offsets), o) and total > cap  # the true counts
    for a in (aft.row_env, aft.play, aft.reward, vals):
        assert (np_(a)[cap:] == -7).all()
    for k in ("row_env", "play", "reward"):
        assert torch.equal(getattr(aft, k)[:cap], getattr(full, k)[:cap]), k
    assert torch.equal(vals[:cap].view(torch.int32), vfull[:cap].view(torch.int32))
    # the scratch is kept on the env and grown only when cap grows: 128 B a row
    assert env._look_scratch.numel() == 128 * total
    # cap = 0: the counts alone
    aft0, v0 = env.lookahead_turn_afterstates(net, dice=st["dice"], cap=0)
    assert aft0.cap == 0 and v0.shape == (0,) and np.array_equal(np_(aft0.offsets), o)
    env.close()


def test_one_wave_a_row_and_four_waves_a_row_give_the_same_bits(states):
    """A launch over at most 3,072 rows splits a row's rolls over four waves,
    a longer one keeps a wave a row: cap = 3,073 on the same 65 envs takes
    the second kernel, whose values must be the first's bit for bit."""
    st = states
    env = _env(st)
    net, _ = nets(SIGMOID80, env.device)
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    total, cap = aft.cap, SPLIT_ROWS + 1
    assert 0 < total <= SPLIT_ROWS
    out, vals = _sentinel_out(env.device, cap, cap)
    wide, v = env.lookahead_turn_afterstates(net, dice=st["dice"], out=(out, vals))
    assert wide.cap == cap and torch.equal(wide.offsets, aft.offsets)
    assert torch.equal(v[:total].view(torch.int32), values.view(torch.int32))
    for a, b in ((out.row_env, aft.row_env), (out.play, aft.play), (out.reward, aft.reward)):
        assert torch.equal(a[:total], b) and (np_(a)[total:] == -7).all()
    assert (np_(vals)[total:] == -7).all()  # rows that do not exist are not touched
    env.close()


def test_nodoubles_takes_the_15_roll_mean(states):
    st = states
    env = _env(st, dice_mode="nodoubles")
    net, cpu = nets(SIGMOID80, env.device)
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    c = row_replies("nodoubles", st, aft, "nodoubles")
    assert len(c["ks"]) == 15
    want, E = expected(cpu, c)
    check(values, want, E, c["live"], "nodoubles")
    all36 = _env(st)
    v36 = all36.lookahead_turn_afterstates(net, dice=st["dice"])[1]
    assert float((values - v36).abs().max()) > 1e3 * TOL_FACTOR * E  # not the 36-roll mean
    all36.close()
    env.close()


def test_graph_replay_reads_the_live_weights(states):
    """The call captured once; l1.weight changed in place and pack()ed; one
    replay gives the eager call's bits for the new weights."""
    st = states
    env = _env(st)
    dev = env.device
    net, _ = nets(SIGMOID80, dev)
    d = torch.as_tensor(st["dice"], dtype=torch.uint8, device=dev).contiguous()
    first, v_old = env.lookahead_turn_afterstates(net, dice=d)  # (workspace and scratch are made here, outside capture)
    cap = first.cap
    out, vals = _sentinel_out(dev, cap, cap)
    v_old = v_old.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            env.lookahead_turn_afterstates(net, dice=d, out=(out, vals))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    torch.manual_seed(100)
    with torch.no_grad():
        net.l1.weight.add_(torch.randn(80, 198, device=dev) * 0.5)
    net.pack()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = vals.clone()
    eager = env.lookahead_turn_afterstates(net, dice=d)[1]
    assert torch.equal(out.offsets, first.offsets) and torch.equal(out.play, first.play)
    assert torch.equal(got.view(torch.int32), eager.view(torch.int32))
    assert not torch.equal(got, v_old)
    env.close()


def test_lookahead_player_plays_the_reference_best():
    """LookaheadPlayer.step() over 5 plies at B = 65 on a FULL4 env: for every
    env the row the float64 reference ranks best; where the reference's two
    best differ by less than 8 E either is accepted, for at most 5 % of the
    (env, ply) pairs."""
    from gym_narde.value_play import LookaheadPlayer, ValuePlayer
    from gym_narde.vector import VecNardeEnv

    B = 65
    env = VecNardeEnv(B, device="cuda:0", seed=2027, rules="full4")
    net, cpu = nets(SIGMOID80, env.device)
    player = LookaheadPlayer(env, net)
    assert isinstance(player, ValuePlayer) and player.plies == 2 and player.fused and player.perspective == "white"
    env.selfplay(40)  # into the middle game
    pairs = close = 0
    for ply in range(5):
        s = env.get_state()
        st = dict(board=np_(s["board"]), off=np_(s["off"]), ft=np_(s["first_turn"]), player=np_(s["player"]),
                  dice=np_(env.dice()))
        black = st["player"] == -1
        rows = env.scored_turn_afterstates(net, dice=st["dice"])[0]
        c = row_replies(None, st, rows)
        want, E = expected(cpu, c)
        full = terminal_outcomes(st, rows).astype(np.float64)
        full[c["live"]] = want
        obs, reward, term, trunc, info, aft, values, actions = player.step()
        assert aft.feat is None and torch.equal(aft.offsets, rows.offsets) and torch.equal(aft.play, rows.play)
        o, row = np_(aft.offsets), np_(info["row"]).astype(np.int64)
        # the wiring: the pick is pick_turn's on the kernel's values
        assert np.array_equal(row, _pick_ref(o, aft.cap, np_(values), black, "white"))
        assert ((row >= 0) == (np.diff(o) > 0)).all()
        has = torch.from_numpy(row >= 0)
        assert torch.equal(actions[has], aft.play[torch.from_numpy(row[row >= 0])])  # the row's play is played
        for e in np.nonzero(row >= 0)[0]:
            seg = full[o[e]:o[e + 1]]
            order = np.argsort(seg if black[e] else -seg, kind="stable")
            pairs += 1
            if row[e] - o[e] == order[0]:
                continue
            assert len(order) > 1 and row[e] - o[e] == order[1], (ply, int(e))
            assert abs(seg[order[0]] - seg[order[1]]) < TOL_FACTOR * E, (ply, int(e))
            close += 1
    print(f"(env, ply) pairs: {pairs}, under the 8 E exemption: {close}")
    assert pairs > 4 * B and close <= 0.05 * pairs
    env.close()


def test_lookahead_player_on_ref2_plays_value_player_two_plies():
    """The same player on a REF2 env: ValuePlayer(plies=2)'s values, rows and
    actions bit for bit."""
    from gym_narde.value_play import LookaheadPlayer, ValuePlayer
    from gym_narde.vector import VecNardeEnv

    a = VecNardeEnv(65, device="cuda:0", seed=31)
    b = VecNardeEnv(65, device="cuda:0", seed=31)
    net, _ = nets(SIGMOID80, a.device)
    pa, pb = LookaheadPlayer(a, net), ValuePlayer(b, net, plies=2)
    for x in (a, b):
        x.selfplay(30)
    for _ in range(3):
        ra, rb = pa.step(), pb.step()
        assert torch.equal(ra[6].view(torch.int32), rb[6].view(torch.int32))  # values
        assert torch.equal(ra[7], rb[7]) and torch.equal(ra[4]["row"], rb[4]["row"])  # actions, rows
        assert torch.equal(ra[0], rb[0])
    a.close()
    b.close()


def test_errors():
    from gym_narde import _lib
    from gym_narde._lib import NardeValueError
    from gym_narde.value_play import LookaheadPlayer
    from gym_narde.vector import VecNardeEnv

    ref2 = VecNardeEnv(4, device="cuda:0")
    net, _ = nets(SIGMOID80, ref2.device)
    with pytest.raises(ValueError, match="full4"):
        ref2.lookahead_turn_afterstates(net)
    ref2.close()
    env = VecNardeEnv(4, device="cuda:0", rules="full4")
    with pytest.raises(TypeError, match="ValueMLP"):
        env.lookahead_turn_afterstates(torch.nn.Sequential())
    with pytest.raises(TypeError, match="ValueMLP"):
        LookaheadPlayer(env, torch.nn.Sequential())
    # the scratch through the C call: too small for cap rows, misaligned
    dev = env.device
    offsets = torch.zeros(5, dtype=torch.int32, device=dev)
    v = torch.zeros(8, dtype=torch.float32, device=dev)
    scratch = torch.empty(128 * 8 + 16, dtype=torch.uint8, device=dev)
    mlp = net.struct()
    args = lambda s, nbytes: (None, 8, _lib.ptr(offsets), None, None, None, ctypes.byref(mlp), 1, _lib.ptr(v), s,  # noqa: E731
                              nbytes, env._s())
    with pytest.raises(NardeValueError, match="scratch_bytes"):
        env.handle.call("narde_turn_afterstates_lookahead", *args(_lib.ptr(scratch), 128 * 8 - 1))
    with pytest.raises(NardeValueError, match="16-B aligned"):
        env.handle.call("narde_turn_afterstates_lookahead", *args(ctypes.c_void_p(scratch.data_ptr() + 8), 128 * 8))
    env.handle.call("narde_turn_afterstates_lookahead", *args(_lib.ptr(scratch), 128 * 8))
    torch.cuda.synchronize()
    env.close()
