"""Playout-greedy play on the GPU (k_aft_fill_records, k_turn_fill_records,
k_rows_topk, k_playout_pick through VecNardeEnv.recorded_afterstates(),
recorded_turn_afterstates(), top_rows(), pick_playout() and
value_play.PlayoutPlayer).

B = 100 envs (a partial fill block, short envs, an env with no row, the four
endgames; FULL4: big_state() last, on an id whose first roll is 1-1 -- the slab
tier, 2,065 rows).  The records' oracle is a second env of R envs set_state()-ed
to the rows' parents and stepped once with each row's codes or play, auto-reset
off: records[0] of a one-ply records rollout of it.  The narrow outputs and
values are scored_afterstates()' / scored_turn_afterstates()' bits, the top-K a
stable torch.sort, the pick tests/test_playout_pick_cpu.py's float64
restatement (exact: integers, one division, one rounding).
"""
import copy

import numpy as np
import pytest

from fuzz_positions import random_positions
from test_afterstates_cpu import golden_states
from test_playout_pick_cpu import numpy_pick
from test_value_cpu import make_net
from test_value_playout_cpu import late_races
from test_value_rollout_cpu import endgames
from turn_afterstates_ref import BIG_ROWS, big_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20251022
B = 100
H128 = (128, "sigmoid", "sigmoid", 2)
H1 = (1, "tanh", "none", 3)
H80 = (80, "sigmoid", "sigmoid", 1)
RULES = ("ref2", "full4")
TRIALS, PLIES = 4, 6
NONE6 = 0xFF


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def np_(x):
    return x.detach().cpu().numpy()


def make_env(n, rules, seed=SEED, id_base=0, max_steps=1000, autoreset=True):
    from gym_narde.vector import VecNardeEnv

    return VecNardeEnv(n, device="cuda:0", seed=seed, env_id_offset=id_base, max_episode_steps=max_steps,
                       autoreset=autoreset, rules=rules)


_NETS = {}


def gpu_net(spec):
    if spec not in _NETS:
        _NETS[spec] = copy.deepcopy(make_net(*spec)).to("cuda:0")
    return _NETS[spec]


def positions(rules):
    """95 golden and fuzz positions, the four endgames, and a last one:
    big_state() under FULL4, one more fuzz position under REF2."""
    g = [np.asarray(a)[::97][:35] for a in golden_states()[:4]]
    f = random_positions(62, 17)[:4]
    e = endgames()
    parts = [g, tuple(a[:60] for a in f), e]
    if rules == "full4":
        b = big_state()
        parts.append((b["board"][None], b["off"][None], b["ft"][None], np.array([b["player"]], np.int8)))
    else:
        parts.append(tuple(a[60:61] for a in f))
    st = tuple(np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    assert st[0].shape[0] == B
    return (st[0].astype(np.int8), st[1].astype(np.uint8), st[2].astype(np.uint8), st[3].astype(np.int8))


_SETUPS = {}


def setup(rules):
    """(env, state, dice): the module's env of B envs; under FULL4 its last
    env's id is one whose first roll is 1-1."""
    if rules not in _SETUPS:
        id_base = 0
        if rules == "full4":
            probe = make_env(4096, rules)
            ones = np.flatnonzero((np_(probe.dice()) == 1).all(1))
            ones = ones[ones >= B - 1]
            assert len(ones), "no env of the probe rolls 1-1 first: choose another seed"
            id_base = int(ones[0]) - (B - 1)
            probe.close()
        env = make_env(B, rules, id_base=id_base)
        state = positions(rules)
        env.set_state(*(torch.as_tensor(a).to(env.device) for a in state))
        dice = env.dice().clone()
        if rules == "full4":
            assert np_(dice)[B - 1].tolist() == [1, 1]
        _SETUPS[rules] = (env, state, dice)
    return _SETUPS[rules]


def recorded(env, net, dice, cap=None, **kw):
    return (env.recorded_turn_afterstates if env.full else env.recorded_afterstates)(net, dice, cap=cap, **kw)


def scored(env, net, dice, cap=None):
    return (env.scored_turn_afterstates if env.full else env.scored_afterstates)(net, dice, cap=cap)


def column(aft):
    return aft.play if hasattr(aft, "play") else aft.codes


def snapshot(env):
    return ({k: np_(v).copy() for k, v in env.get_state().items()}, np_(env.stats()).copy(), int(env.ply))


def assert_untouched(env, before, what):
    after = snapshot(env)
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), (what, k)
    assert np.array_equal(before[1], after[1]) and before[2] == after[2], what


def test_the_inputs_hold_the_cases_that_matter():
    for rules in RULES:
        env, state, dice = setup(rules)
        aft = (env.turn_afterstates if env.full else env.afterstates)(dice, feat=False)
        rows = np.diff(np_(aft.offsets))
        assert (rows == 0).any() and ((rows >= 1) & (rows < 3)).any() and (rows > 8).any(), rules
        assert (np_(aft.reward) != 0).any(), rules
        if rules == "full4":
            assert rows[B - 1] == BIG_ROWS


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("spec", [H1, H128, None], ids=["H1", "H128", "no-net"])
def test_records_are_the_stepped_envs_records(rules, spec):
    env, state, dice = setup(rules)
    net = gpu_net(spec) if spec is not None else None
    before = snapshot(env)
    aft, values, records = recorded(env, net, dice)
    assert_untouched(env, before, "recorded")
    R = aft.cap
    assert records.dtype == torch.int32 and tuple(records.shape) == (R, 8) and records.data_ptr() % 16 == 0
    # the narrow outputs and the values: the scored expansion's bits
    ref_net = net if net is not None else gpu_net(H80)
    saft, svalues = scored(env, ref_net, dice)
    assert saft.cap == R
    for k in ("offsets", "row_env", "reward"):
        assert torch.equal(getattr(aft, k), getattr(saft, k)), k
    assert torch.equal(column(aft), column(saft))
    if net is None:
        assert values is None
    else:
        assert torch.equal(values.view(torch.int32), svalues.view(torch.int32))
    # the oracle: R envs at the rows' parents, stepped once with each row's action, auto-reset off
    parent = aft.row_env.long()
    two = make_env(R, rules, seed=1, max_steps=1000, autoreset=False)
    two.set_state(*(torch.as_tensor(a).to(env.device)[parent] for a in state))
    two.ply = env.ply
    _, rew, term, _, _ = two.step(column(aft), dice=dice[parent])
    assert torch.equal(rew.to(torch.int8), aft.reward) and torch.equal(term != 0, aft.reward != 0)
    one = gpu_net(H80)
    if rules == "full4":
        bufs = two.turn_value_rollout_buffers(1, dice=False, play=False, value=False, records=True)
        two.turn_value_rollout(1, one, bufs=bufs)
    else:
        bufs = two.value_rollout_buffers(1, dice=False, actions=False, value=False, records=True)
        two.value_rollout(1, one, bufs=bufs)
    want = np_(bufs["records"][0])
    got = np_(records)
    assert np.array_equal(got, want)
    assert (got[:, 7] == env.ply + 1).all() and ((got[:, 6].view(np.uint32) >> 16) == 1).all()
    two.close()
    # cap given: the same rows below it, nothing at or past it, the true counts
    cap = R // 2
    col = column(aft)
    out = (type(aft)(torch.empty_like(aft.offsets), torch.full((R,), -7, dtype=torch.int32, device=env.device),
                     torch.full_like(col, -7), None, None, torch.full((R,), -7, dtype=torch.int8, device=env.device), R),
           None if net is None else torch.full((R,), 5.0, device=env.device),
           torch.full((R, 8), -7, dtype=torch.int32, device=env.device))
    caft, cvalues, crec = recorded(env, net, dice, cap=cap, out=out)
    assert caft.cap == cap and torch.equal(caft.offsets, aft.offsets)
    assert torch.equal(crec, records[:cap]) and (out[2][cap:] == -7).all()
    assert torch.equal(column(caft)[:cap], col[:cap]) and (column(out[0])[cap:] == -7).all()
    assert (out[0].row_env[cap:] == -7).all() and (out[0].reward[cap:] == -7).all()
    if net is not None:
        assert torch.equal(cvalues.view(torch.int32), values[:cap].view(torch.int32)) and (out[1][cap:] == 5.0).all()


def sorted_topk(offsets, cap, value, black, perspective, k):
    """torch.sort(stable=True) per env: NaNs first in row order, then the best
    value, the lowest row on ties."""
    off = offsets.tolist()
    sel = torch.full((len(off) - 1, k), -1, dtype=torch.int32)
    v = value.cpu().double()
    for e in range(len(off) - 1):
        r0, r1 = off[e], min(off[e + 1], cap)
        if r1 <= r0:
            continue
        x = -v[r0:r1] if (perspective == "white" and black[e]) else v[r0:r1]
        key = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), -x)
        order = torch.sort(key, stable=True).indices[:k]
        sel[e, :len(order)] = (r0 + order).to(torch.int32)
    return sel


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_top_rows_are_the_stable_sort_and_the_picks_row(rules, k):
    env, state, dice = setup(rules)
    black = state[3] == -1
    aft, values, records = recorded(env, gpu_net(H128), dice)
    R = aft.cap
    rows = np.diff(np_(aft.offsets))
    wide = int(np.argmax(rows[:B - 1]))
    r0 = int(aft.offsets[wide])
    nans = values.clone()
    nans[[r0 + 1, r0 + 3]] = float("nan")
    pick = env.pick_turn if env.full else env.pick_afterstate
    before = snapshot(env)
    none = torch.zeros(8, dtype=torch.int32)
    none[6] = NONE6
    for name, v in (("net", values), ("all-ties", torch.zeros_like(values)), ("nans", nans)):
        for perspective in ("white", "mover"):
            for cap in (R, r0 + 2):
                a = aft._replace(cap=cap)
                sel, roots = env.top_rows(a, v, k, records, perspective)
                want = sorted_topk(aft.offsets, cap, v, black, perspective, k)
                assert torch.equal(sel.cpu(), want), (name, perspective, cap)
                _, row = pick(a, v, perspective)
                assert torch.equal(sel[:, 0], row), (name, perspective, cap)
                flat = sel.reshape(-1).long().cpu()
                rc, rt = records.cpu(), roots.cpu()
                assert tuple(roots.shape) == (B * k, 8)
                assert torch.equal(rt[flat >= 0], rc[flat[flat >= 0]])
                assert (rt[flat < 0] == none).all()
                alone, nothing = env.top_rows(a, v, k, None, perspective)
                assert nothing is None and torch.equal(alone, sel)
    assert_untouched(env, before, "top_rows")
    # any row stride of the values, as the picks take it
    wide_v = torch.stack([values, values + 1.0], 1)
    sel2, _ = env.top_rows(aft, wide_v[:, 0], k)
    sel1, _ = env.top_rows(aft, values, k)
    assert torch.equal(sel1, sel2)


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("leaf", [False, True], ids=["finished-mean", "truncated-mean"])
def test_pick_playout_is_the_float64_restatement(rules, k, leaf):
    env, state, dice = setup(rules)
    net = gpu_net(H128)
    black = (state[3] == -1).astype(np.uint8)
    before = snapshot(env)
    aft, values, records = recorded(env, net, dice)
    sel, roots = env.top_rows(aft, values, k, records)
    res = env.playout(roots, TRIALS, net, max_plies=PLIES, seed=SEED + 1, common_dice=True, leaf=True, per_trial=True)
    actions, row, score = env.pick_playout(aft, values, sel, res, leaf=leaf)
    assert_untouched(env, before, "the chain")
    sums, lf = np_(res.sums), np_(res.leaf)
    want_row, want_score = numpy_pick(np_(sel), np_(values), np_(aft.reward), sums, lf if leaf else None, TRIALS, black)
    assert np.array_equal(np_(score).view(np.uint32), want_score.view(np.uint32))
    assert np.array_equal(np_(row), want_row)
    has = want_row >= 0
    col = np_(column(aft))
    assert np.array_equal(np_(actions)[has], col[want_row[has]])
    assert (np_(actions)[~has] == (-1 if env.full else 0)).all() and (~has).any()
    # the tuple form of the result
    tup = (res.sums, TRIALS, res.leaf) if leaf else (res.sums, TRIALS)
    a2, r2, s2 = env.pick_playout(aft, values, sel, tup, leaf=leaf)
    assert torch.equal(a2, actions) and torch.equal(r2, row) and torch.equal(s2.view(torch.int32), score.view(torch.int32))
    # both ends are in the inputs: unfinished live roots and the endgames' terminal rows
    flat = np_(sel).reshape(-1)
    live = (flat >= 0) & (np_(aft.reward)[np.maximum(flat, 0)] == 0)
    assert (sums[live, 0] < TRIALS).any() and ((flat >= 0) & ~live).any()


@pytest.mark.parametrize("rules", RULES)
def test_a_finishing_case(rules):
    """Late races and the endgames at max_plies 40 (tests/test_value_playout_cpu.py's
    finishing case: the CPU oracle shows every trial finished)."""
    state = tuple(np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(late_races(), endgames()))
    env = make_env(8, rules, seed=4)
    env.set_state(*(torch.as_tensor(a).to(env.device) for a in state))
    net = gpu_net(H80)
    dice = env.dice()
    aft, values, records = recorded(env, net, dice)
    k = 3
    sel, roots = env.top_rows(aft, values, k, records)
    res = env.playout(roots, 5, net, max_plies=40, seed=17, common_dice=True, leaf=True)
    actions, row, score = env.pick_playout(aft, values, sel, res)
    flat = np_(sel).reshape(-1)
    live = (flat >= 0) & (np_(aft.reward)[np.maximum(flat, 0)] == 0)
    assert live.any() and (np_(res.finished)[live] == 5).all()
    want_row, want_score = numpy_pick(np_(sel), np_(values), np_(aft.reward), np_(res.sums), None, 5,
                                      (state[3] == -1).astype(np.uint8))
    assert np.array_equal(np_(row), want_row)
    assert np.array_equal(np_(score).view(np.uint32), want_score.view(np.uint32))
    # a live slot's score is its finished trials' mean outcome
    sc = np_(score).reshape(-1)
    assert np.allclose(sc[live], np_(res.points)[live] / 5.0)
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_playout_player_with_one_candidate_is_the_value_player(rules):
    from gym_narde.value_play import PlayoutPlayer, ValuePlayer

    net = gpu_net(H80)
    a, b = make_env(B, rules, seed=7), make_env(B, rules, seed=7)
    pp = PlayoutPlayer(a, net, k=1, trials=2, max_plies=3, seed=5)
    vp = ValuePlayer(b, net)
    for ply in range(8):
        oa = pp.step()
        ob = vp.step()
        assert torch.equal(oa[7], ob[7]), f"actions ply {ply}"
        assert torch.equal(oa[1], ob[1]) and torch.equal(oa[2], ob[2]), f"reward ply {ply}"
        assert torch.equal(oa[4]["row"], ob[4]["row"]) and torch.equal(oa[4]["sel"][:, 0], ob[4]["row"])
        assert tuple(oa[4]["score"].shape) == (B, 1) and oa[4]["playout"].trials == 2
    sa, sb = a.get_state(), b.get_state()
    assert all(torch.equal(sa[key], sb[key]) for key in sa) and a.ply == b.ply == 8
    a.close()
    b.close()


@pytest.mark.parametrize("rules", RULES)
def test_playout_player_picks_among_candidates(rules):
    """k = 4 with cap given: the move played is the pick's, a row of the env's top 4."""
    from gym_narde.value_play import PlayoutPlayer

    env = make_env(B, rules, seed=9)
    pp = PlayoutPlayer(env, gpu_net(H80), k=4, trials=TRIALS, max_plies=PLIES, cap=B * 64, truncated=True, seed=3)
    for _ in range(3):
        out = pp.step()
        info, aft, actions = out[4], out[5], out[7]
        row, sel = info["row"].long(), info["sel"].long()
        has = row >= 0
        assert has.any() and (sel == row[:, None])[has].any(1).all()
        assert torch.equal(actions[has], column(aft)[row[has]])
    assert pp._ply == env.ply
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_the_five_calls_replay_from_one_graph(rules):
    env = make_env(B, rules, seed=11)
    env.set_state(*(torch.as_tensor(a).to(env.device) for a in positions(rules)))
    net = copy.deepcopy(make_net(*H80)).to(env.device)
    net.pack()
    k, cap = 3, 4096
    t = torch
    dev = env.device

    def chain(env, bufs=None):
        dice = env.dice()
        aft, values, records = recorded(env, net, dice, cap=cap, out=None if bufs is None else bufs["rows"])
        sel, roots = env.top_rows(aft, values, k, records, out=None if bufs is None else bufs["top"])
        res = env.playout(roots, TRIALS, net, max_plies=PLIES, seed=SEED, common_dice=True, leaf=True,
                          out=None if bufs is None else bufs["res"])
        pick = env.pick_playout(aft, values, sel, res, leaf=True, out=None if bufs is None else bufs["pick"])
        step = env.step(pick[0])
        return dict(rows=(aft, values, records), top=(sel, roots), res=res, pick=pick, step=step)

    # eager, on a twin env: the first ply's results and the state it leaves (the FULL4 workspaces are made here)
    twin = make_env(B, rules, seed=11)
    twin.set_state(*(t.as_tensor(a).to(dev) for a in positions(rules)))
    eager = chain(twin)
    t.cuda.synchronize()
    want = dict(actions=eager["pick"][0].clone(), score=eager["pick"][2].clone(), sums=eager["res"].sums.clone(),
                state={k_: v.clone() for k_, v in twin.get_state().items()})
    bufs = chain(env)  # outside capture once: the arrays the graph writes, and the handle's workspaces
    t.cuda.synchronize()
    env.set_state(*(t.as_tensor(a).to(dev) for a in positions(rules)))
    env.ply = 0
    for x in (bufs["pick"][0], bufs["res"].sums):
        x.fill_(-3)
    g = t.cuda.CUDAGraph()
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        with t.cuda.graph(g, stream=side):
            chain(env, bufs)
    t.cuda.current_stream().wait_stream(side)
    g.replay()
    t.cuda.synchronize()
    assert t.equal(bufs["pick"][0], want["actions"]) and t.equal(bufs["res"].sums, want["sums"])
    assert t.equal(bufs["pick"][2].view(t.int32), want["score"].view(t.int32))
    st = env.get_state()
    assert all(t.equal(st[k_], want["state"][k_]) for k_ in st)
    # the replay sees weights changed in place: the second ply under the new net is the twin's eager one
    with t.no_grad():
        other = make_net(*H80[:3], 9).to(dev)
        for p, q in zip(net.parameters(), other.parameters()):
            p.copy_(q)
    net.pack()
    eager2 = chain(twin)
    t.cuda.synchronize()
    g.replay()
    t.cuda.synchronize()
    assert t.equal(bufs["pick"][0], eager2["pick"][0]) and t.equal(bufs["res"].sums, eager2["res"].sums)
    assert t.equal(bufs["rows"][1].view(t.int32)[:64], eager2["rows"][1].view(t.int32)[:64])
    assert not t.equal(eager2["rows"][1][:64], eager["rows"][1][:64])
    env.close()
    twin.close()


@pytest.mark.parametrize("rules", RULES)
def test_the_example_plays_by_playouts(rules, capsys):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("play_value_agent", os.path.join(ROOT, "examples", "play_value_agent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ep, white, black = mod.main(envs=32, plies=4, device="cuda:0", rules=rules, playout=2, top=2)
    assert ep == 0 and white == 0 and black == 0  # four plies from the start position end no game
    assert "played out 2 times each" in capsys.readouterr().out
    with pytest.raises(ValueError):
        mod.main(envs=8, plies=1, device="cuda:0", rules=rules, playout=2, depth=2)
