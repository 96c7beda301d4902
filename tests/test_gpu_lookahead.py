"""The two-ply lookahead on the GPU (k_aft_fill_rec and k_aft_look through
VecNardeEnv.lookahead_afterstates and ValuePlayer(plies=2); DESIGN.md section
17): the structural outputs bit for bit against scored_afterstates(), the
values against the float64 reference pipeline of tests/lookahead_ref.py
within tol = 8 x E, E = max |pipeline in torch float32 - in float64| on the
same rows, floored at one float32 ulp of the largest magnitude compared
(tests/test_lookahead_cpu.py states the argument); terminal rows exact.

The reference uses only calls that existed before the lookahead: a second env
holding the rows' records (set_state to the rows' parents, step(codes, dice)
with autoreset off), afterstates(feat=True) on it per roll, and for a roll
with no reply the position step((0, 0), roll) leaves.
"""
import copy
import ctypes

import numpy as np
import pytest

from test_afterstates_cpu import golden_states, reference_afterstates
from test_value_cpu import TOL_FACTOR, make_net

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import lookahead_ref as LR  # noqa: E402
from afterstate_checks import _env, _pick_ref, np_  # noqa: E402
from test_gpu_afterstates import _first  # noqa: E402

SIGMOID80 = (80, "sigmoid", "sigmoid", 1)
NETS = [(1, "relu", "none", 3), (17, "tanh", "none", 6), SIGMOID80, (128, "sigmoid", "sigmoid", 2)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def case():
    st = golden_states()
    return st, reference_afterstates(*st)


def nets(spec, device):
    """The net on the device and its CPU twin (the reference)."""
    cpu = make_net(*spec)
    return copy.deepcopy(cpu).to(device), cpu


def row_replies(st, aft, dice_mode="all36"):
    """The rows' records on a second env, and per roll the live rows' replies.
    st: (board, off, first_turn, player, dice) of the envs (tensors or
    arrays); aft: their rows.  Returns (live mask (R,), black (live,) bool:
    black replies, replies as lookahead_ref.two_ply takes them)."""
    dev = aft.row_env.device
    e = aft.row_env.long()
    parent = [torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dev)[e] for a in st]
    rows = _env(parent[:4], dice_mode=dice_mode)
    rows.step(aft.codes, parent[4])
    rec = rows.get_state()
    live = np_(aft.reward) == 0
    assert np.array_equal(np_(rows.terminated) != 0, ~live)
    idx = torch.from_numpy(np.nonzero(live)[0]).to(dev)
    rec = [rec[k][idx].clone() for k in ("board", "off", "first_turn", "player")]
    rows.close()
    n = len(idx)
    replies = []
    if n:
        lv = _env(rec, dice_mode=dice_mode)
        zero = torch.zeros((n, 2), dtype=torch.int16, device=dev)
        for a, b in LR.rolls_of(dice_mode):
            d = torch.tensor([[a, b]], dtype=torch.uint8, device=dev).repeat(n, 1)
            lv.set_state(*rec)
            r = lv.afterstates(dice=d)
            feat = np_(r.feat)
            rep = dict(offsets=np_(r.offsets), feat=feat, reward=np_(r.reward),
                       player=np.where(feat[:, 197] > 0.5, -1, 1).astype(np.int8))
            lv.step(zero, d)  # no reply: what the step with (0, 0) leaves
            rep.update(pass_feat=np_(lv.tesauro198()), pass_reward=np_(lv.reward).astype(np.int8),
                       pass_player=np_(lv.get_state()["player"]))
            replies.append(rep)
        lv.close()
    return live, np_(rec[3]) == -1, replies


def expected(cpu, st, aft, dice_mode="all36"):
    """(fp64 values of the live rows, E, live mask)."""
    live, black, replies = row_replies(st, aft, dice_mode)
    if live.any():
        want, w32, _ = LR.two_ply(cpu, replies, black)
        E = LR.error_bound(w32, want)
    else:
        want, E = np.zeros(0), 0.0
    return want, E, live


def check(values, want, E, live, what):
    """Live rows within 8 E, terminal rows the outcome exactly."""
    got = np_(values)
    err = float(np.abs(got[live].astype(np.float64) - want).max()) if live.any() else 0.0
    print(f"{what}: E = {E:.3e}, max error = {err:.3e} = {err / max(E, 1e-30):.2f} E")
    assert err <= TOL_FACTOR * E, (what, err, TOL_FACTOR * E)
    return err


def terminal_outcomes(st, aft):
    """The terminal rows' outcomes: reward, negated when black made the move."""
    r = np_(aft.reward).astype(np.float32)
    mover = np.asarray(st[3])[np_(aft.row_env)]
    return np.where(mover == -1, -r, r)


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
@pytest.mark.parametrize("B", [1, 65])
def test_rows_and_values(case, B, spec):
    st, _ = _first(case, B)
    env = _env(st)
    net, cpu = nets(spec, env.device)
    one, v1 = env.scored_afterstates(net, dice=st[4])
    aft, values = env.lookahead_afterstates(net, dice=st[4])
    assert aft.feat is None and aft.obs is None and aft.cap == one.cap and values.shape == (one.cap,)
    for k in ("offsets", "row_env", "codes", "reward"):
        assert torch.equal(getattr(aft, k), getattr(one, k)), k
    want, E, live = expected(cpu, st, aft)
    check(values, want, E, live, f"B={B} {spec[:3]}")
    assert np.array_equal(np_(values)[~live], terminal_outcomes(st, aft)[~live])
    assert torch.equal(values[torch.from_numpy(~live)], v1[torch.from_numpy(~live)])
    # not the one-ply values
    assert float((values - v1).abs().max()) > 1e3 * TOL_FACTOR * E
    # the same bits on a second call
    again = env.lookahead_afterstates(net, dice=st[4])[1]
    assert torch.equal(values.view(torch.int32), again.view(torch.int32))
    env.close()


def test_many_workgroups_and_terminal_rows(case):
    """B = 257 (2,400 rows: workgroups beyond a handful), and states whose
    rows end the game for either colour."""
    st, ref = case
    term_env = np.unique(ref["row_env"][ref["reward"] != 0])
    white = [e for e in term_env if st[3][e] == 1][:4]
    black = [e for e in term_env if st[3][e] == -1][:4]
    idx = np.concatenate([np.arange(257 - 8), white, black]).astype(np.int64)
    sub = tuple(np.ascontiguousarray(a[idx]) for a in st)
    env = _env(sub)
    net, cpu = nets(SIGMOID80, env.device)
    aft, values = env.lookahead_afterstates(net, dice=sub[4])
    one, v1 = env.scored_afterstates(net, dice=sub[4])
    for k in ("offsets", "row_env", "codes", "reward"):
        assert torch.equal(getattr(aft, k), getattr(one, k)), k
    want, E, live = expected(cpu, sub, aft)
    assert aft.cap > 2000
    out = terminal_outcomes(sub, aft)
    assert (out[~live] > 0).any() and (out[~live] < 0).any()  # terminal rows of both colours
    check(values, want, E, live, "B=257")
    assert np.array_equal(np_(values)[~live], out[~live])
    env.close()


def test_padded_weight_rows(case):
    """ld_w1t = H + 4 through the C call: the bits of the dense layout."""
    from gym_narde import _lib

    st, _ = _first(case, 65)
    env = _env(st)
    dev = env.device
    for spec in ((17, "tanh", "none", 6), SIGMOID80):
        net, _ = nets(spec, dev)
        aft, values = env.lookahead_afterstates(net, dice=st[4])
        H, cap = net.hidden, aft.cap
        wide = torch.full((198, H + 4), 1e9, dtype=torch.float32, device=dev)  # a read past H would show
        wide[:, :H] = net.l1.weight.detach().t()
        mlp = net.struct()
        mlp.w1t, mlp.ld_w1t = wide.data_ptr(), H + 4
        d = torch.as_tensor(st[4], dtype=torch.uint8, device=dev).contiguous()
        offsets = torch.zeros(66, dtype=torch.int32, device=dev)
        v = torch.zeros(cap, dtype=torch.float32, device=dev)
        scratch = torch.empty(_lib.lookahead_scratch_bytes(cap), dtype=torch.uint8, device=dev)
        env.handle.call("narde_afterstates_lookahead", _lib.ptr(d), cap, _lib.ptr(offsets), None, None, None,
                        ctypes.byref(mlp), 1, _lib.ptr(v), _lib.ptr(scratch), scratch.numel(), env._s())
        assert torch.equal(offsets, aft.offsets)
        assert torch.equal(v.view(torch.int32), values.view(torch.int32))
    env.close()


def test_cap_cuts_values_not_offsets(case):
    from gym_narde.vector import Afterstates

    st, _ = _first(case, 65)
    env = _env(st)
    net, cpu = nets(SIGMOID80, env.device)
    full, vfull = env.lookahead_afterstates(net, dice=st[4])
    o = np_(full.offsets)
    total = int(o[-1])
    e = int(np.nonzero(np.diff(o) >= 5)[0][20])
    cap = int(o[e]) + 2
    assert o[e] < cap < o[e + 1] and cap < total
    dev = env.device
    out = Afterstates(torch.zeros(66, dtype=torch.int32, device=dev),
                      torch.full((total,), -7, dtype=torch.int32, device=dev),
                      torch.full((total, 2), -7, dtype=torch.int16, device=dev), None, None,
                      torch.full((total,), -7, dtype=torch.int8, device=dev), cap)
    vals = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    aft, values = env.lookahead_afterstates(net, dice=st[4], out=(out, vals))
    assert aft.cap == cap and values.shape == (cap,)
    assert np.array_equal(np_(aft.offsets), o) and total > cap  # the true counts
    for a in (aft.row_env, aft.codes, aft.reward, vals):
        assert (np_(a)[cap:] == -7).all()
    for k in ("row_env", "codes", "reward"):
        assert torch.equal(getattr(aft, k)[:cap], getattr(full, k)[:cap]), k
    assert torch.equal(vals[:cap].view(torch.int32), vfull[:cap].view(torch.int32))
    # the scratch is kept on the env and grown only when cap grows
    assert env._look_scratch.numel() == 32 * total
    # cap = 0: the counts alone
    aft0, v0 = env.lookahead_afterstates(net, dice=st[4], cap=0)
    assert aft0.cap == 0 and v0.shape == (0,) and np.array_equal(np_(aft0.offsets), o)
    env.close()


def test_one_wave_a_row_and_four_waves_a_row_give_the_same_bits(case):
    """A launch over at most 3,072 rows splits a row's rolls over four waves,
    a longer one keeps a wave a row: cap = 3,073 on the same 65 envs takes
    the second kernel, whose values must be the first's bit for bit."""
    from gym_narde.vector import Afterstates

    st, _ = _first(case, 65)
    env = _env(st)
    dev = env.device
    net, _ = nets(SIGMOID80, dev)
    aft, values = env.lookahead_afterstates(net, dice=st[4])
    total, cap = aft.cap, 3073
    assert 0 < total <= 3072
    out = Afterstates(torch.zeros(66, dtype=torch.int32, device=dev), torch.full((cap,), -7, dtype=torch.int32, device=dev),
                      torch.full((cap, 2), -7, dtype=torch.int16, device=dev), None, None,
                      torch.full((cap,), -7, dtype=torch.int8, device=dev), cap)
    vals = torch.full((cap,), -7.0, dtype=torch.float32, device=dev)
    wide, v = env.lookahead_afterstates(net, dice=st[4], out=(out, vals))
    assert wide.cap == cap and torch.equal(wide.offsets, aft.offsets)
    assert torch.equal(v[:total].view(torch.int32), values.view(torch.int32))
    for a, b in ((out.row_env, aft.row_env), (out.codes, aft.codes), (out.reward, aft.reward)):
        assert torch.equal(a[:total], b) and (np_(a)[total:] == -7).all()
    assert (np_(vals)[total:] == -7).all()  # rows that do not exist are not touched
    env.close()


def test_nodoubles_takes_the_30_roll_mean(case):
    st, _ = _first(case, 65)
    env = _env(st, dice_mode="nodoubles")
    net, cpu = nets(SIGMOID80, env.device)
    aft, values = env.lookahead_afterstates(net, dice=st[4])
    want, E, live = expected(cpu, st, aft, "nodoubles")
    check(values, want, E, live, "nodoubles")
    all36 = _env(st)
    v36 = all36.lookahead_afterstates(net, dice=st[4])[1]
    assert float((values - v36).abs().max()) > 1e3 * TOL_FACTOR * E  # not the 36-roll mean
    all36.close()
    env.close()


def test_graph_replay_reads_the_live_weights(case):
    """The call captured once; l1.weight changed in place and pack()ed; one
    replay gives the eager call's bits for the new weights."""
    from gym_narde.vector import Afterstates

    st, _ = _first(case, 65)
    env = _env(st)
    dev = env.device
    net, _ = nets(SIGMOID80, dev)
    d = torch.as_tensor(st[4], dtype=torch.uint8, device=dev).contiguous()
    first, v_old = env.lookahead_afterstates(net, dice=d)  # (the scratch is made here, outside capture)
    cap = first.cap
    out = Afterstates(torch.zeros(66, dtype=torch.int32, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev),
                      torch.zeros((cap, 2), dtype=torch.int16, device=dev), None, None,
                      torch.zeros(cap, dtype=torch.int8, device=dev), cap)
    vals = torch.zeros(cap, dtype=torch.float32, device=dev)
    v_old = v_old.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            env.lookahead_afterstates(net, dice=d, out=(out, vals))
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
    eager = env.lookahead_afterstates(net, dice=d)[1]
    assert torch.equal(out.offsets, first.offsets) and torch.equal(out.codes, first.codes)
    assert torch.equal(got.view(torch.int32), eager.view(torch.int32))
    assert not torch.equal(got, v_old)
    env.close()


def test_value_player_two_plies_plays_the_reference_best():
    """ValuePlayer(plies=2).step() over 5 plies at B = 65: for every env the
    row the float64 reference ranks best; where the reference's two best
    differ by less than 8 E either is accepted, for at most 5 % of the (env,
    ply) pairs."""
    from gym_narde.value_play import ValuePlayer
    from gym_narde.vector import VecNardeEnv

    B = 65
    env = VecNardeEnv(B, device="cuda:0", seed=2027)
    net, cpu = nets(SIGMOID80, env.device)
    player = ValuePlayer(env, net, plies=2)
    assert player.plies == 2 and player.fused and ValuePlayer(env, net).plies == 1
    env.selfplay(40)  # into the middle game
    pairs = close = 0
    for ply in range(5):
        s = env.get_state()
        st = (s["board"].clone(), s["off"].clone(), s["first_turn"].clone(), s["player"].clone(), env.dice().clone())
        black = np_(st[3]) == -1
        rows = env.scored_afterstates(net, dice=st[4])[0]
        want, E, live = expected(cpu, [np_(a) for a in st], rows)
        full = terminal_outcomes([np_(a) for a in st], rows).astype(np.float64)
        full[live] = want
        obs, reward, term, trunc, info, aft, values, actions = player.step()
        assert aft.feat is None and torch.equal(aft.offsets, rows.offsets) and torch.equal(aft.codes, rows.codes)
        o, row = np_(aft.offsets), np_(info["row"]).astype(np.int64)
        # the wiring: the pick is pick_afterstate's on the kernel's values
        assert np.array_equal(row, _pick_ref(o, aft.cap, np_(values), black, "white"))
        assert ((row >= 0) == (np.diff(o) > 0)).all()
        has = torch.from_numpy(row >= 0)
        assert torch.equal(actions[has], aft.codes[torch.from_numpy(row[row >= 0])])  # the row's codes are played
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


def test_errors():
    from gym_narde.value_play import ValuePlayer
    from gym_narde.vector import VecNardeEnv

    full = VecNardeEnv(4, device="cuda:0", rules="full4")
    net, _ = nets(SIGMOID80, full.device)
    with pytest.raises(ValueError, match="ref2"):
        full.lookahead_afterstates(net)
    with pytest.raises(ValueError, match="ref2"):
        ValuePlayer(full, net, plies=2)
    full.close()
    env = VecNardeEnv(4, device="cuda:0")
    with pytest.raises(ValueError, match="white"):
        ValuePlayer(env, net, perspective="mover", plies=2)
    with pytest.raises(ValueError, match="fused"):
        ValuePlayer(env, net, fused=False, plies=2)
    with pytest.raises(TypeError, match="ValueMLP"):
        ValuePlayer(env, torch.nn.Sequential(), plies=2)
    with pytest.raises(ValueError, match="plies"):
        ValuePlayer(env, net, plies=3)
    with pytest.raises(TypeError, match="ValueMLP"):
        env.lookahead_afterstates(torch.nn.Sequential())
    env.close()
