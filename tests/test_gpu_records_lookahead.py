"""Two-ply values of given records and the pick over given slot scores on the
GPU (the look kernels' second instantiations, k_turn_look_pack and k_slot_pick
through VecNardeEnv.lookahead_records() and pick_slots(); DESIGN.md section
25), both rule sets.

Oracles: on the public records of a roll's rows the existing full lookahead,
bit for bit; on given positions the float64 pipelines of
tests/lookahead_ref.py / tests/turn_lookahead_ref.py over the C oracle within
TOL_FACTOR (8) x E, E the reference's own float32-vs-float64 rounding floored
at one ulp (tests/test_records_lookahead_cpu.py builds both); for the pick its
numpy restatement and pick_playout() with zero sums, one trial and the scores
as leaves.
"""
import ctypes

import numpy as np
import pytest

import lookahead_ref as LR
import test_records_lookahead_cpu as C
import turn_lookahead_ref as TL
from test_gpu_playout_pick import B, H1, H80, H128, RULES, assert_untouched, column, gpu_net, make_env, np_, positions
from test_gpu_playout_pick import recorded, snapshot
from test_value_cpu import TOL_FACTOR, make_net

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H17 = (17, "tanh", "none", 6)
NETS = [H1, H17, H80, H128]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(x):
    return x.contiguous().view(torch.int32)


def full_search(env, net, dice, cap=None):
    return (env.lookahead_turn_afterstates if env.full else env.lookahead_afterstates)(net, dice, cap=cap)


def fixed_dice(n, seed=1):
    d = np.random.default_rng(seed).integers(1, 7, (n, 2)).astype(np.uint8)
    d[-1] = (6, 5)  # (FULL4: big_state() last -- no 2,065-row double here)
    return d


def env_of(rules, st, dice_mode="all36", seed=11):
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(len(st[3]), device="cuda:0", seed=seed, dice_mode=dice_mode, rules=rules)
    env.set_state(*(torch.as_tensor(a).to(env.device) for a in st))
    return env


# ------------------------------------------------------------------ 1. the rows' records against the full search
@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"H{s[0]}")
@pytest.mark.parametrize("n_envs", [1, 65])
def test_rows_records_give_the_full_searchs_bits(rules, spec, n_envs):
    st = positions(rules)
    dice = fixed_dice(B)
    pick = slice(0, 1) if n_envs == 1 else slice(B - 65, B)  # the last 65 hold the four endgames
    st, dice = tuple(a[pick] for a in st), torch.as_tensor(dice[pick]).to("cuda:0")
    env = env_of(rules, st)
    net = gpu_net(spec)
    aft, two = full_search(env, net, dice)
    aft2, one, records = recorded(env, net, dice)
    assert aft2.cap == aft.cap and torch.equal(aft2.offsets, aft.offsets) and aft.cap >= 1
    live = aft.reward == 0
    if n_envs == 65:  # the inputs hold the cases: terminal rows of both colours beside live ones, an env with no row
        assert int((~live).sum()) >= 4 and int(live.sum()) > 300
        assert (np.diff(np_(aft.offsets)) == 0).any()
    before, rec0 = snapshot(env), records.clone()
    got = env.lookahead_records(records, net)
    torch.cuda.synchronize()
    assert got.shape == (aft.cap,) and got.dtype == torch.float32
    assert torch.equal(bits(got[live]), bits(two[live]))
    assert torch.isnan(got[~live]).all() and not torch.isnan(got[live]).any()
    assert torch.equal(records, rec0)
    assert_untouched(env, before, "lookahead_records")
    assert torch.equal(bits(env.lookahead_records(records, net)), bits(got))  # the same bits on every call
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_one_record_300_records_and_past_the_split(rules):
    """n = 3,073 takes one wave a record, n <= 3,072 four: the same bits; a
    sentinel past value[n] is intact."""
    st = positions(rules)
    env = env_of(rules, st)
    net = gpu_net(H80)
    _, _, records = recorded(env, net, torch.as_tensor(fixed_dice(B)).to(env.device))
    assert records.shape[0] >= 300
    many = records.repeat(-(-3073 // records.shape[0]), 1)[:3073].contiguous()
    # the ply counter and elapsed words of the long launch's copies differ from the short ones'
    many[:, 7] += 12345
    many[:, 6] += 3 << 16
    big = torch.full((3073 + 8,), -7.0, dtype=torch.float32, device=env.device)
    wide = env.lookahead_records(many, net, out=big[:3073])
    assert wide.data_ptr() == big.data_ptr() and (np_(big)[3073:] == -7).all()
    for n in (1, 300):
        small = torch.full((n + 8,), -7.0, dtype=torch.float32, device=env.device)
        env.lookahead_records(records[:n].contiguous(), net, out=small[:n])
        assert (np_(small)[n:] == -7).all()
        assert torch.equal(bits(small[:n]), bits(big[:n]))
    assert not torch.isnan(big[:300]).all()
    env.close()


# ------------------------------------------------------------------ 2. given positions against the CPU reference
def check(got, want, w32, what):
    E = LR.error_bound(w32, want)
    err = float(np.abs(np_(got).astype(np.float64) - want).max())
    print(f"{what}: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E")
    assert np.ptp(want) > 1e3 * TOL_FACTOR * E
    assert err <= TOL_FACTOR * E, (err, TOL_FACTOR * E)
    return E


_REF = {}


def reference(rules):
    if rules not in _REF:
        if rules == "ref2":
            rec = C.positions2()
            _REF[rules] = (rec, C.replies2(rec, "all36"), None)
        else:
            rec = C.positions4()
            _REF[rules] = (rec,) + C.replies4(rec, "all36")
    return _REF[rules]


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("spec", [H17, H128], ids=lambda s: f"H{s[0]}")
def test_given_positions_against_the_cpu_reference(rules, spec):
    rec, replies, ks = reference(rules)
    black = rec[3] == -1
    cpu = make_net(*spec)
    net = gpu_net(spec)
    out = {}
    for mode in ("all36", "nodoubles"):
        env = env_of(rules, tuple(a[:2] for a in rec), dice_mode=mode)  # (the env's own positions play no part)
        records = env.state_records(*rec, t=4242)
        before = snapshot(env)
        got = env.lookahead_records(records, net)
        torch.cuda.synchronize()
        assert_untouched(env, before, "lookahead_records")
        if rules == "ref2":
            keep = [i for i, (a, b) in enumerate(LR.rolls_of("all36")) if mode == "all36" or a != b]
            want, w32, _ = LR.two_ply(cpu, [replies[i] for i in keep], black)
            assert len(keep) == (36 if mode == "all36" else 30)
        else:
            kk = TL.rolls_of(mode)
            want, w32, _ = TL.two_ply_weighted(cpu, [replies[ks.index(k)] for k in kk], kk, black)
            assert len(kk) == (21 if mode == "all36" else 15)
        out[mode] = (got, want, check(got, want, w32, f"{rules} H{spec[0]} {mode}"))
        env.close()
    # NODOUBLES is not the all-rolls mean
    assert float((out["all36"][0] - out["nodoubles"][0]).abs().max()) > 1e3 * TOL_FACTOR * out["nodoubles"][2]


def test_overflow_tier_records_full4():
    """A record whose 1-1 reply outgrows the 2,048-node tier (the slab), four
    whose replies outgrow the 256-node frontier (the LDS tier), an ordinary
    one: the redone rolls enter the values, which are within 8 E; the ordinary
    record's bits are those it gets alone."""
    cs = [TL.reference_case(TL.tier_state(p)) for p in (TL.TIER_SLAB_POINTS, TL.TIER_LDS_POINTS)]
    cnt = [np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1) for c in cs]
    assert cnt[0].shape[0] == 1 and cnt[0][0, 0] > 2048  # the tiers are reached
    assert cnt[1].shape[0] == 4 and 256 < cnt[1].max() <= 2048
    plain = tuple(a[:1] for a in C.positions4())
    env = env_of("full4", plain)
    cpu, net = make_net(*H17), gpu_net(H17)
    rec = tuple(np.concatenate([cs[0]["rec"][i], cs[1]["rec"][i], plain[i]]) for i in range(4))
    got = env.lookahead_records(env.state_records(*rec, t=9), net)
    for c, sl in ((cs[0], slice(0, 1)), (cs[1], slice(1, 5))):
        want, w32, _ = TL.two_ply_weighted(cpu, c["replies"], c["ks"], c["rec"][3] == -1)
        E = LR.error_bound(w32, want)
        err = float(np.abs(np_(got[sl]).astype(np.float64) - want).max())
        print(f"tier records {sl}: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E")
        assert err <= TOL_FACTOR * E
    alone = env.lookahead_records(env.state_records(*plain), net)
    assert torch.equal(bits(alone), bits(got[5:]))
    env.close()


def test_finished_records_are_nan():
    for rules in RULES:
        env = make_env(4, rules)
        net = gpu_net(H80)
        board = np.zeros((3, 24), np.int8)
        off = np.array([[15, 3], [0, 15], [14, 14]], np.uint8)
        board[0, 13], board[1, 5], board[2, 0], board[2, 14] = -12, 15, 1, -1
        rec = env.state_records(board, off, np.zeros((3, 2), np.uint8), np.array([1, -1, 1], np.int8), t=7)
        none = torch.tensor([[0, 0, 0, 0, 0, 0, 0xFF, 0]], dtype=torch.int32, device=env.device)
        got = np_(env.lookahead_records(torch.cat([rec, none]), net))
        assert np.isnan(got[[0, 1, 3]]).all() and np.isfinite(got[2])
        env.close()


# ------------------------------------------------------------------ 4. the slot pick
@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_pick_slots_is_the_numpy_restatement_and_the_playout_pick_of_one_leaf(rules, k):
    env = env_of(rules, positions(rules))
    net = gpu_net(H80)
    aft, values, records = recorded(env, net, torch.as_tensor(fixed_dice(B)).to(env.device))
    sel, _ = env.top_rows(aft, values, k, records)
    rng = np.random.default_rng(k)
    score = rng.choice(np.linspace(-1, 1, 5).astype(np.float32), (B, k))  # few levels: ties
    black = (positions(rules)[3] == -1).astype(np.uint8)
    col = np_(column(aft)).reshape(aft.cap, -1).view(np.uint32)
    c = dict(n=B, k=k, cap=aft.cap, word=col.shape[1] * 4, sel=np_(sel), value=np_(values), reward=np_(aft.reward),
             column=col, black=black)
    assert (c["sel"] < 0).all(1).any() and (c["reward"][np.maximum(c["sel"], 0)][c["sel"] >= 0] != 0).any()
    for with_nan in (False, True):
        s = score.copy()
        if with_nan:
            s[rng.random(s.shape) < 0.15] = np.nan
        dev = torch.as_tensor(s).to(env.device)
        actions, row, sc = env.pick_slots(aft, values, sel, dev)
        wout, wrow, wsc, _ = C.numpy_slot_pick(c, s)
        assert np.array_equal(np_(row), wrow)
        assert np.array_equal(np_(actions).reshape(B, -1).view(np.uint32), wout)
        g = np_(sc)
        assert np.array_equal(np.isnan(g), np.isnan(wsc)) and np.array_equal(g[~np.isnan(g)], wsc[~np.isnan(wsc)])
        if not with_nan:  # pick_playout() with zero sums, one trial and the scores as leaves: (0 + leaf) / 1
            sums = torch.zeros((B * k, 4), dtype=torch.int32, device=env.device)
            pa, pr, ps = env.pick_playout(aft, values, sel, (sums, 1, dev.reshape(B * k, 1).contiguous()), leaf=True)
            assert torch.equal(pa, actions) and torch.equal(pr, row)
            assert torch.equal(torch.isnan(ps), torch.isnan(sc)) and torch.equal(bits(ps.nan_to_num(9.0)), bits(sc.nan_to_num(9.0)))
    env.close()


# ------------------------------------------------------------------ 5. the pruned player
@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_pruned_player_plays_the_best_of_the_top_rows_by_the_full_search(rules, k):
    from gym_narde.value_play import LookaheadPlayer

    st = positions(rules)
    env, twin = env_of(rules, st), env_of(rules, st)
    net = gpu_net(H80)
    dice = env.dice().clone()
    aft, two = full_search(env, net, dice)
    aft1, one, records = recorded(env, net, dice)
    sel, _ = env.top_rows(aft1, one, k, records)
    out = LookaheadPlayer(env, net, top=k).step()
    full = LookaheadPlayer(twin, net).step()
    info, actions = out[4], out[7]
    torch.cuda.synchronize()
    assert torch.equal(info["sel"], sel) and torch.equal(info["dice"], dice)
    s, v, rows = np_(sel), np_(two), np.diff(np_(aft.offsets))
    want = np.full(B, -1, np.int64)
    for e in range(B):
        cand = [(i, float(v[s[e, i]])) for i in range(k) if s[e, i] >= 0]
        if cand:
            x = [(-sc if st[3][e] == -1 else sc) for _, sc in cand]
            want[e] = s[e, cand[int(np.argmax(x))][0]]  # (np.argmax: the first of equals, the lowest slot)
    assert np.array_equal(np_(info["row"]), want)
    assert (want == -1).any() and (rows > k).any() and (k == 1 or ((rows >= 1) & (rows <= k)).any())
    # the slots' scores: the full search's values of the selected rows
    sc = np_(info["score"])
    assert np.array_equal(sc[s >= 0].view(np.uint32), v[s[s >= 0]].view(np.uint32)) and np.isnan(sc[s < 0]).all()
    # envs with at most k rows: the unpruned player's row and action
    few = torch.as_tensor(rows <= k).to(env.device)
    assert torch.equal(info["row"][few], full[4]["row"][few]) and torch.equal(actions[few], full[7][few])
    col = column(aft)
    has = info["row"] >= 0
    assert torch.equal(actions[has], col[info["row"][has].long()])
    env.close()
    twin.close()


@pytest.mark.parametrize("rules", RULES)
def test_top_1_plays_the_value_players_moves(rules):
    from gym_narde.value_play import LookaheadPlayer, ValuePlayer

    a, b = make_env(B, rules, seed=3), make_env(B, rules, seed=3)
    net = gpu_net(H80)
    pa, pb = LookaheadPlayer(a, net, top=1), ValuePlayer(b, net)
    for ply in range(20):
        x, y = pa.step(), pb.step()
        assert torch.equal(x[7], y[7]) and torch.equal(x[4]["row"], y[4]["row"]), ply
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
    sa, sb = a.get_state(), b.get_state()
    assert all(torch.equal(sa[key], sb[key]) for key in sa)
    a.close()
    b.close()


# ------------------------------------------------------------------ 6. graph replay
@pytest.mark.parametrize("rules", RULES)
def test_the_five_calls_replay_from_one_graph(rules):
    import copy

    t = torch
    env, twin = (make_env(B, rules, seed=11) for _ in range(2))
    for e in (env, twin):
        e.set_state(*(t.as_tensor(a).to(e.device) for a in positions(rules)))
    dev = env.device
    net = copy.deepcopy(make_net(*H80)).to(dev)
    net.pack()
    k, cap = 3, 4096

    def chain(env, bufs=None):
        dice = env.dice()
        aft, values, records = recorded(env, net, dice, cap=cap, out=None if bufs is None else bufs["rows"])
        sel, roots = env.top_rows(aft, values, k, records, out=None if bufs is None else bufs["top"])
        two = env.lookahead_records(roots, net, out=None if bufs is None else bufs["two"])
        pick = env.pick_slots(aft, values, sel, two.view(B, k), out=None if bufs is None else bufs["pick"])
        step = env.step(pick[0])
        return dict(rows=(aft, values, records), top=(sel, roots), two=two, pick=pick, step=step)

    eager = chain(twin)  # (the FULL4 workspaces and scratch are made in these calls, outside capture)
    t.cuda.synchronize()
    want = dict(actions=eager["pick"][0].clone(), score=eager["pick"][2].clone(), two=eager["two"].clone(),
                state={k_: v.clone() for k_, v in twin.get_state().items()})
    bufs = chain(env)
    t.cuda.synchronize()
    env.set_state(*(t.as_tensor(a).to(dev) for a in positions(rules)))
    env.ply = 0
    bufs["pick"][0].fill_(-3)
    bufs["two"].fill_(-3)
    g = t.cuda.CUDAGraph()
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        with t.cuda.graph(g, stream=side):
            chain(env, bufs)
    t.cuda.current_stream().wait_stream(side)
    g.replay()
    t.cuda.synchronize()
    same = lambda a, b: t.equal(bits(a.nan_to_num(9.0)), bits(b.nan_to_num(9.0))) and t.equal(a.isnan(), b.isnan())  # noqa: E731
    assert t.equal(bufs["pick"][0], want["actions"]) and same(bufs["two"], want["two"])
    assert same(bufs["pick"][2], want["score"])
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
    assert t.equal(bufs["pick"][0], eager2["pick"][0]) and same(bufs["two"], eager2["two"])
    assert not same(eager2["two"], eager["two"])
    env.close()
    twin.close()


# ------------------------------------------------------------------ 7. the learner
def make_learner(rules, net_seed=9):
    import copy

    from gym_narde.td import LookaheadTargetLearner

    env = make_env(64, rules, seed=5)
    net = copy.deepcopy(make_net(80, "sigmoid", "tanh", seed=net_seed)).to(env.device)
    return LookaheadTargetLearner(env, net, alpha=0.002, plies=4, every=2, epsilon=0.1, seed=3)


def weight_bits(net):
    return [bits(p.detach()).clone() for p in net.parameters()] + [bits(net._w1t).clone()]


@pytest.mark.parametrize("rules", RULES)
def test_lookahead_target_learner(rules):
    from gym_narde.td import ValueFitter

    a, b, c = (make_learner(rules) for _ in range(3))
    N = 2 * 64
    # targets(): the two-ply values of the window's positions of every second ply
    a.play()
    target, weight = a.targets()
    recs = a.bufs["records"][::2].reshape(N, 8).contiguous()
    want = a.env.lookahead_records(recs, a.net)
    nan = torch.isnan(want)
    assert target.shape == weight.shape == (N,) and torch.equal(a.roots, recs)
    assert torch.equal(torch.isnan(target), nan) and torch.equal(bits(target[~nan]), bits(want[~nan]))
    assert torch.equal(weight, (~nan).float()) and int((~nan).sum()) > 0
    loss = a.update()
    assert loss.shape == (2,) and float(loss[1]) == float((~nan).sum())
    # one step() = ValueFitter.step on those arrays
    b.play()
    b.targets()
    ValueFitter(b.env, b.net, N).step(b.roots, b.target, b.weight, alpha=b.alpha)
    torch.cuda.synchronize()
    for x, y in zip(weight_bits(a.net), weight_bits(b.net)):
        assert torch.equal(x, y)
    assert not torch.equal(weight_bits(a.net)[0], bits(make_net(80, "sigmoid", "tanh", seed=9).l1.weight.detach()).to(x.device))
    # two learners with the same arguments agree after 3 steps
    c.step()
    for _ in range(2):
        a.step()
        c.step()
    torch.cuda.synchronize()
    for x, y in zip(weight_bits(a.net), weight_bits(c.net)):
        assert torch.equal(x, y)
    assert a.windows == 3 and a.memory_bytes() > 32 * N and a.values().shape == (N,)
    for lr in (a, b, c):
        lr.env.close()


# ------------------------------------------------------------------ 8. errors
def test_errors():
    from gym_narde.td import LookaheadTargetLearner
    from gym_narde.value_play import LookaheadPlayer

    env = make_env(8, "ref2")
    dev, net = env.device, gpu_net(H80)
    rec = env.state_records(*(a[:8] for a in positions("ref2")))
    for bad in (rec.float(), rec[:, :7].contiguous(), rec[::2], rec[:0], rec.cpu(), np_(rec)):
        with pytest.raises(ValueError):
            env.lookahead_records(bad, net)
    with pytest.raises(TypeError):
        env.lookahead_records(rec, torch.nn.Linear(198, 1).to(dev))
    for bad in (torch.zeros(7, device=dev), torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(8)):
        with pytest.raises(ValueError):
            env.lookahead_records(rec, net, out=bad)
    aft, values, records = env.recorded_afterstates(net)
    sel, roots = env.top_rows(aft, values, 2, records)
    ok = torch.zeros((8, 2), device=dev)
    for bad_sel, bad_score in ((sel.long(), ok), (sel[:4], ok), (sel, ok.double()), (sel, torch.zeros((8, 3), device=dev)),
                               (sel, ok.cpu()), (sel, torch.zeros((2, 8), device=dev))):
        with pytest.raises(ValueError):
            env.pick_slots(aft, values, bad_sel, bad_score)
    env.pick_slots(aft, values, sel, ok.reshape(16))  # (B * k,) is accepted
    for top in (0, 65, -1):
        with pytest.raises(ValueError):
            LookaheadPlayer(env, net, top=top)
    for top in (2.5, "3", True):
        with pytest.raises(TypeError):
            LookaheadPlayer(env, net, top=top)
    with pytest.raises(TypeError):
        LookaheadPlayer(env, torch.nn.Linear(198, 1).to(dev), top=2)
    with pytest.raises(ValueError):
        LookaheadPlayer(env, net, top=2).step(epsilon=torch.tensor(0.1, device=dev), tag=torch.tensor(0, device=dev))
    for kw in (dict(plies=0), dict(plies=4, every=0)):
        with pytest.raises(ValueError):
            LookaheadTargetLearner(env, net, alpha=0.1, **kw)
    with pytest.raises(TypeError):
        LookaheadTargetLearner(env, torch.nn.Linear(198, 1).to(dev), alpha=0.1, plies=4)
    # the C call's own checks behind the Python layer: a scratch one byte short
    full = make_env(8, "full4")
    from gym_narde import _lib

    frec = full.state_records(*(a[:8] for a in positions("full4")))
    v = torch.zeros(8, device=dev)
    scratch = torch.empty(128 * 8, dtype=torch.uint8, device=dev)
    mlp = net.struct()
    with pytest.raises(Exception, match="NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES"):
        full.handle.call("narde_turn_records_lookahead", 8, _lib.ptr(frec), ctypes.byref(mlp), _lib.ptr(v),
                         _lib.ptr(scratch), 128 * 8 - 1, full._s())
    full.close()
    env.close()


# ------------------------------------------------------------------ 9. the examples
def _example(name):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rules", RULES)
def test_the_examples_run_with_the_new_flags(rules, capsys, tmp_path):
    ep, white, black = _example("play_value_agent").main(envs=32, plies=4, device="cuda:0", rules=rules, depth=2, top=2)
    assert ep == 0 and white == 0 and black == 0  # four plies from the start position end no game
    assert "the best 2 searched two plies deep" in capsys.readouterr().out
    with pytest.raises(ValueError):
        _example("play_value_agent").main(envs=8, plies=1, device="cuda:0", rules=rules, top=2)
    path = str(tmp_path / "agent.pt")
    _example("train_value_agent").main(envs=32, plies=8, hidden=17, rules=rules, out=path, device="cuda:0", window=4,
                                       lookahead_targets=True, every=2)
    assert "rms error" in capsys.readouterr().out
    sd = torch.load(path, map_location="cpu")
    assert sd["l1.weight"].shape == (17, 198) and torch.isfinite(sd["l1.weight"]).all()
    with pytest.raises(SystemExit):
        _example("train_value_agent").main(envs=8, plies=4, device="cuda:0", lookahead_targets=True)
