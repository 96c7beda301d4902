"""The FULL4 value rollout (narde_turn_value_rollout: k_turn_value_rollout,
DESIGN.md section 20) on the CPU, through a test-only host build that runs
the kernel's shared functions serially
(tests/hostcheck/hostcheck_turn_value_rollout.cpp), replayed ply by ply over
the C oracle.

The replay is teacher-forced: the run records dice and plays, the reference
walks the same plies with those plays (O.full4_turn with the pick words that
select them, the TimeLimit and the auto-reset restated as in
test_value_rollout_cpu.py) and judges every ply on its own, so one near-tie
cannot make the rest of a game incomparable.  A greedy ply is right if its
play is a row of enumerate_turns for that position and roll, and that row is
the reference's arg-best (the lowest row on ties) whenever the reference's
best beats its runner-up by more than 8 E in float64; otherwise its reference
value must be within 8 E of the best.  E = lookahead_ref.error_bound of the
pipeline in torch float32 against float64 over the rows compared.  At most
1 % of the greedy (env, ply) pairs may fall under the exemption, which is
computed from the reference alone; each test prints the count.  Explore plies
and random plies match exactly.
"""
import copy
import ctypes
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT
from lookahead_ref import error_bound
from turn_afterstates_ref import BIG_ROWS, big_state, edge_states, enumerate_turns, selfplay_states

torch = pytest.importorskip("torch")

from test_value_cpu import TOL_FACTOR, make_net, outcome  # noqa: E402
from test_value_rollout_cpu import (BLACK, ENV0, M32, NETS, PICK_SEED, SEED, TAG, P, endgames, mulhi,  # noqa: E402
                                    net_in, ply_words, reset_black)

STRIDE, PLIES, ROOM = 53, 6, 256
SEARCH = 2000  # ply counters tried for a wanted first roll (a roll has probability >= 1/36)


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_turn_value_rollout.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_turn_value_rollout.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    assert lib.hc_turn_rollout_piece() == 83536  # narde.h's NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1)
    return lib


def roll_of(t, env):
    k36 = mulhi(ply_words(t, env)[0], 36)
    return k36 // 6 + 1, k36 % 6 + 1


def t_for_roll(e, want, start):
    """The first ply counter >= start at which env e rolls `want` (in order)."""
    for t in range(start, start + SEARCH):
        if roll_of(t, ENV0 + e) == want:
            return t
    raise AssertionError(f"no ply counter gives env {e} the roll {want}")


def start_positions():
    """The start position, white and black to move, under 3-3, 4-4, 6-6 (two
    head moves on the first turn) and 5-3."""
    rolls = [(3, 3), (4, 4), (6, 6), (5, 3)] * 2
    board = np.zeros((8, 24), np.int8)
    board[:, 23], board[:, 11] = 15, -15
    return dict(board=board, off=np.zeros((8, 2), np.uint8), ft=np.ones((8, 2), np.uint8),
                player=np.array([1] * 4 + [-1] * 4, np.int8), dice=np.array(rolls, np.uint8))


def start_states():
    """(board, off, ft, player, elapsed, t): a stride of the FULL4 golden
    states, the self-play states, the edge states, the start position, the
    endgames and big_state().  Every env's ply counter is chosen (O.philox)
    so that its first roll is the one its set records -- the edge states' M = 1
    and pass cases and big_state()'s 1-1 are cases of a roll --, from a start
    that varies with the env."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "full4.npz"))
    gold = {k: np.asarray(g[k])[::STRIDE] for k in ("board", "off", "ft", "player", "dice")}
    eb, eo, ef, ep = endgames()
    ends = dict(board=eb, off=eo, ft=ef, player=ep, dice=np.array([[6, 5], [2, 2], [4, 1], [3, 3]], np.uint8))
    big = {k: np.asarray(v)[None] for k, v in big_state().items()}
    sets = [gold, selfplay_states(), edge_states(), start_positions(), ends, big]
    board, off, ft, player, dice = (np.ascontiguousarray(np.concatenate([np.asarray(s[k]) for s in sets]))
                                    for k in ("board", "off", "ft", "player", "dice"))
    n = board.shape[0]
    t = np.zeros(n, np.uint32)
    for e in range(n):
        d = (int(dice[e, 0]), int(dice[e, 1]))
        ok = 1 <= d[0] <= 6 and 1 <= d[1] <= 6  # (the edge states' two bad rolls: any roll)
        t[e] = t_for_roll(e, d, e % 7) if ok else e % 7
    return (board.astype(np.int8), off.astype(np.uint8), ft.astype(np.uint8), player.astype(np.int8),
            np.zeros(n, np.uint16), t)


def host_rollout(hc, st, white, black, plies=PLIES, max_steps=1000, eps=None, room=ROOM):
    board, off, ft, player, elapsed, t = (a.copy() for a in st)
    n = board.shape[0]
    stats = np.zeros((n, 3), np.int32)
    keep = []
    o = dict(dice=np.zeros((plies, n, 2), np.uint8), play=np.zeros((plies, n, 4, 2), np.int8),
             value=np.zeros((plies, n), np.float32), reward=np.zeros((plies, n), np.int32),
             terminated=np.zeros((plies, n), np.uint8), truncated=np.zeros((plies, n), np.uint8),
             words=np.zeros((plies, n, 4), np.uint32), rows=np.zeros((plies, n), np.int32),
             row=np.zeros((plies, n), np.int32), explored=np.zeros((plies, n), np.uint8),
             tier=np.zeros((plies, n), np.uint8), front=np.zeros((plies, n), np.int32),
             mdice=np.zeros((plies, n), np.int32))
    w, b = net_in(white, keep), net_in(black, keep)
    hc.hc_turn_value_rollout(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(elapsed), P(t), P(stats),
                             ctypes.c_int64(ENV0), ctypes.c_uint64(SEED), 0, max_steps, plies, room, ctypes.byref(w),
                             ctypes.byref(b), int(eps is not None), ctypes.c_float(0.0 if eps is None else eps),
                             ctypes.c_uint64(PICK_SEED), ctypes.c_int64(TAG),
                             *(P(o[k]) for k in ("dice", "play", "value", "reward", "terminated", "truncated", "words",
                                                 "rows", "row", "explored", "tier", "front", "mdice")))
    o["final"] = dict(board=board, off=off, ft=ft, player=player, elapsed=elapsed, t=t, stats=stats)
    return o


def popcount(m):
    m = np.asarray(m, np.uint64)
    return sum(((m >> np.uint64(p)) & np.uint64(1)).astype(np.int64) for p in range(24))


def forced_turn(board, off, ft, player, dice, play):
    """The oracle's turn that plays `play` (n,4,2): sub-move k's pick word is
    the smallest that selects the play's entry of the oracle's C_k (list
    order: the higher die's sources ascending, then the lower die's).  A
    sub-move that is not in C_k fails."""
    n = len(player)
    words = np.zeros((n, 4), np.uint32)
    dh = dice.max(1).astype(np.int64)
    for k in range(4):
        r = O.full4_turn(board, off, ft, player, dice, words)
        live = np.flatnonzero((r["max_dice"].astype(np.int64) > k) & (play[:, k, 0] >= 0))
        if not len(live):
            break
        src, die = play[live, k, 0].astype(np.uint64), play[live, k, 1].astype(np.int64)
        ch, cl = r["cmask"][live, k, 0].astype(np.uint64), r["cmask"][live, k, 1].astype(np.uint64)
        hi = die == dh[live]
        mask = np.where(hi, ch, cl)
        assert (((mask >> src) & np.uint64(1)) == 1).all(), f"sub-move {k} is not in the oracle's C_{k}"
        idx = np.where(hi, 0, popcount(ch)) + popcount(mask & ((np.uint64(1) << src) - np.uint64(1)))
        nc = popcount(ch) + popcount(cl)
        words[live, k] = ((idx.astype(np.uint64) << np.uint64(32)) + (nc - 1).astype(np.uint64)) // nc.astype(np.uint64)
    r = O.full4_turn(board, off, ft, player, dice, words)
    assert np.array_equal(r["played"], play), "the oracle plays another turn than the recorded one"
    return r


def turn_words(words):
    """narde_rules.h turn_words: the four pick words of a FULL4 turn from the ply's words."""
    r1, r2 = words[:, 1].astype(np.uint64), words[:, 2].astype(np.uint64)
    return np.stack([r1, r2, (r1 * 0x85EBCA6B) & M32, (r2 * 0xC2B2AE35) & M32], 1).astype(np.uint32)


def ref_values(net, feat):
    x = torch.from_numpy(np.ascontiguousarray(feat))
    with torch.no_grad():
        return net(x).double().numpy().reshape(-1), copy.deepcopy(net).double()(x.double()).numpy().reshape(-1)


def replay(hc, st, out, white, black, plies=PLIES, max_steps=1000, eps=None):
    """Walk the recorded plies over the oracle.  Exact things are asserted
    here; returns what the float judgement needs."""
    sp = O.SelfPlay(1)
    sp.reset(0)
    start_board, start_off, start_ft = sp.board[0].copy(), sp.off[0].copy(), sp.ft[0].copy()
    board, off, ft, player, elapsed, t = (a.copy() for a in st)
    n = board.shape[0]
    stats = np.zeros((n, 3), np.int32)
    J = dict(gap=[], is_best=[], short=[], verr=[], E=0.0, norow=0, explored=0, random=0, greedy=0,
             terminal_pick={1: 0, -1: 0}, wins={1: 0, 2: 0}, resets=0, four=0, m1_high=0, heads=0, big=0)
    eps_q = None if eps is None else int(min(max(float(np.float32(eps)), 0.0), 1.0) * 4294967296.0)
    for k in range(plies):
        words = np.array([ply_words(int(t[e]), ENV0 + e) for e in range(n)], np.uint32)
        assert np.array_equal(words, out["words"][k]), f"ply {k}: words"
        k36 = (words[:, 0].astype(np.uint64) * 36) >> 32
        dice = np.stack([k36 // 6 + 1, k36 % 6 + 1], 1).astype(np.uint8)
        assert np.array_equal(dice, out["dice"][k]), f"ply {k}: dice"
        play = out["play"][k]
        has = np.array([(white if p == 1 else black) is not None for p in player])
        ref = enumerate_turns(board, off, ft, player, dice)
        offs = ref["offsets"]
        v32, v64 = {}, {}
        for colour, net in ((1, white), (-1, black)):
            if net is not None and len(ref["reward"]):
                a, b = ref_values(net, ref["feat"])
                term = ref["reward"] != 0
                oc = outcome(ref["reward"], ref["player"], "white").astype(np.float64)
                v32[colour], v64[colour] = np.where(term, oc, a), np.where(term, oc, b)
        # a colour with no net: the host build's env_ply_full random step, bit for bit
        rnd = np.flatnonzero(~has)
        if len(rnd):
            b1, o1, f1, p1 = (np.ascontiguousarray(x[rnd]).copy() for x in (board, off, ft, player))
            el1, t1 = np.ascontiguousarray(elapsed[rnd]).copy(), np.ascontiguousarray(t[rnd]).copy()
            s1 = np.zeros((len(rnd), 3), np.int32)
            pl1, rw1 = np.zeros((len(rnd), 4, 2), np.int8), np.zeros(len(rnd), np.int32)
            tm1, tr1 = np.zeros(len(rnd), np.uint8), np.zeros(len(rnd), np.uint8)
            for j, e in enumerate(rnd):  # (env ids differ: one env a call)
                sl = slice(j, j + 1)
                hc.hc_turn_random_ply(ctypes.c_int64(1), P(b1[sl]), P(o1[sl]), P(f1[sl]), P(p1[sl]), P(el1[sl]),
                                      P(t1[sl]), P(s1[sl]), ctypes.c_int64(ENV0 + int(e)), ctypes.c_uint64(SEED), 0,
                                      max_steps, P(pl1[sl]), P(rw1[sl]), P(tm1[sl]), P(tr1[sl]))
            assert np.array_equal(pl1, play[rnd]), f"ply {k}: random plays"
            assert np.array_equal(rw1, out["reward"][k][rnd]) and np.array_equal(tm1, out["terminated"][k][rnd])
            assert np.array_equal(tr1, out["truncated"][k][rnd])
            assert np.isnan(out["value"][k][rnd]).all() and (out["rows"][k][rnd] == -1).all()
            J["random"] += len(rnd)
            # and the oracle's turn under the ply's pick words
            ro = O.full4_turn(board[rnd], off[rnd], ft[rnd], player[rnd], dice[rnd], turn_words(words[rnd]))
            assert np.array_equal(ro["played"], play[rnd]), f"ply {k}: random plays against the oracle"
        for e in np.flatnonzero(has):
            r0, r1 = int(offs[e]), int(offs[e + 1])
            assert out["rows"][k, e] == r1 - r0, f"ply {k} env {e}: row count"
            if r1 == r0:
                J["norow"] += 1
                assert (play[e] == -1).all() and np.isnan(out["value"][k, e]) and out["row"][k, e] == -1
                continue
            hit = np.nonzero((ref["play"][r0:r1] == play[e][None]).all((1, 2)))[0]
            assert len(hit) == 1, f"ply {k} env {e}: play {play[e].tolist()} is not a row"
            j = int(hit[0])
            assert out["row"][k, e] == j
            colour = int(player[e])
            x64 = v64[colour][r0:r1] * (1.0 if colour == 1 else -1.0)
            explore = False
            if eps_q is not None:
                r = O.philox(((TAG + k) & M32, e, 0, 5), (PICK_SEED & M32, PICK_SEED >> 32))
                explore = r[0] < eps_q
                if explore:
                    J["explored"] += 1
                    assert j == mulhi(r[1], r1 - r0), f"ply {k} env {e}: explore row"
            assert bool(out["explored"][k, e]) == explore
            J["E"] = max(J["E"], error_bound(v32[colour][r0:r1], v64[colour][r0:r1]))
            J["verr"].append(abs(float(out["value"][k, e]) - float(v64[colour][r0 + j])))
            if ref["reward"][r0 + j] != 0:
                J["terminal_pick"][colour] += 1
            d0, d1 = int(dice[e, 0]), int(dice[e, 1])
            nsub = int((play[e, :, 0] >= 0).sum())
            J["four"] += int(d0 == d1 and nsub == 4)
            J["m1_high"] += int(d0 != d1 and ref["max_dice"][e] == 1 and play[e, 0, 1] == max(d0, d1))
            J["heads"] += int(d0 == d1 and d0 in (3, 4, 6) and int((play[e, :, 0] == 23).sum()) == 2)
            J["big"] += int(r1 - r0 == BIG_ROWS)
            if not explore:
                J["greedy"] += 1
                jb = int(np.argmax(x64))
                rest = np.delete(x64, jb)
                J["gap"].append(float(x64[jb] - rest.max()) if len(rest) else np.inf)
                J["is_best"].append(j == jb)
                J["short"].append(float(x64[jb] - x64[j]))
        # the step, the TimeLimit, the statistics, the auto-reset
        stp = forced_turn(board, off, ft, player, dice, play)
        rew = stp["reward"].astype(np.int32)
        term = stp["done"].astype(np.uint8)
        assert np.array_equal(rew, out["reward"][k]) and np.array_equal(term, out["terminated"][k]), f"ply {k}: step"
        assert np.array_equal(stp["max_dice"].astype(np.int32), out["mdice"][k]), f"ply {k}: max dice"
        elapsed = elapsed + 1
        trunc = ((max_steps > 0) & (elapsed >= max_steps)).astype(np.uint8)
        assert np.array_equal(trunc, out["truncated"][k]), f"ply {k}: truncated"
        for e in np.nonzero(term)[0]:
            J["wins"][int(rew[e])] += 1
            stats[e, 1 if player[e] == 1 else 2] += rew[e]
        player = np.where(term != 0, player, -player).astype(np.int8)
        board, off, ft = stp["board"], stp["off"], stp["first_turn"]
        for e in np.nonzero(term | trunc)[0]:
            stats[e, 0] += 1
            J["resets"] += 1
            board[e], off[e], ft[e], elapsed[e] = start_board, start_off, start_ft, 0
            player[e] = -1 if reset_black(words[e, 3]) else 1
        t = t + 1
    fin = out["final"]
    for name, a in (("board", board), ("off", off), ("ft", ft), ("player", player), ("elapsed", elapsed), ("t", t),
                    ("stats", stats)):
        assert np.array_equal(fin[name].astype(np.int64), np.asarray(a).astype(np.int64)), f"final {name}"
    return J


def judge(J, what):
    tol = TOL_FACTOR * J["E"]
    gap, is_best, short, verr = (np.array(J[k]) for k in ("gap", "is_best", "short", "verr"))
    clear = gap > tol
    exempt = int((~clear).sum())
    print(f"{what}: {J['greedy']} greedy, {J['explored']} explore, {J['random']} random, {J['norow']} pass plies; "
          f"E = {J['E']:.3e}; exempt (gap <= 8 E) {exempt}; max |value - ref| = {verr.max() if len(verr) else 0:.3e}")
    assert is_best[clear].all(), "a clear best was not played"
    assert (short[~clear] <= tol).all(), "a near-tie's row is not within 8 E of the best"
    assert exempt <= 0.01 * max(1, J["greedy"])
    assert (verr <= tol).all(), (verr.max(), tol)
    return exempt


@pytest.fixture(scope="module")
def st():
    return start_states()


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_greedy_plies_through_the_shared_functions(hc, st, spec):
    white, black = make_net(*spec), make_net(*BLACK[spec[0]])
    out = host_rollout(hc, st, white, black)
    J = replay(hc, st, out, white, black)
    judge(J, f"{spec[:3]} vs {BLACK[spec[0]][:3]}")
    if spec[0] == 80:  # the inputs hold the cases that matter
        assert J["terminal_pick"][1] > 0 and J["terminal_pick"][-1] > 0  # a terminal pick by each colour
        assert J["wins"][1] > 0 and J["wins"][2] > 0
        assert J["norow"] > 0  # passes
        assert J["four"] > 0  # a doubles turn with four sub-moves
        assert J["m1_high"] > 0  # a two-dice turn with M = 1 on the higher die
        assert J["heads"] > 0  # a first-turn 3-3 / 4-4 / 6-6 play with two head moves
        assert J["resets"] > 0  # the auto-reset inside the six plies
        assert (st[3] == -1).any() and (st[3] == 1).any()  # envs that start with black to move
        # big_state() under 1-1: 2,065 rows, past the 256-node tier
        assert J["big"] == 1 and out["rows"][0, -1] == BIG_ROWS and out["tier"][0, -1] == 1
        assert out["front"][0, -1] > ROOM and out["tier"][0, :-1].sum() < 0.01 * st[0].shape[0]
        print(f"plies on the second tier at room {ROOM}: {int(out['tier'].sum())} of {out['tier'].size}")


def test_truncation_resets_and_plays_the_next_episodes_opening(hc, st):
    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    out = host_rollout(hc, st, white, black, max_steps=4)
    quiet = ~out["terminated"].any(0)  # (an env that won on the way restarted its count)
    assert quiet.sum() > 2000 and out["truncated"][3][quiet].all() and not out["truncated"][:3].any()
    assert not out["truncated"][4:][:, quiet].any()
    J = replay(hc, st, out, white, black, max_steps=4)
    judge(J, "max_episode_steps 4")
    assert J["resets"] >= st[0].shape[0]
    assert (out["final"]["elapsed"][quiet] == 2).all() and (out["final"]["stats"][quiet, 0] == 1).all()


@pytest.mark.parametrize("eps", [1.0, 0.3])
def test_explore_plies_are_turn_pick_rows(hc, st, eps):
    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    out = host_rollout(hc, st, white, black, eps=eps)
    J = replay(hc, st, out, white, black, eps=eps)
    judge(J, f"epsilon {eps}")
    if eps == 1.0:
        assert J["greedy"] == 0 and J["explored"] > 10000
    else:
        assert J["greedy"] > 0 and 0.25 < J["explored"] / (J["explored"] + J["greedy"]) < 0.35


@pytest.mark.parametrize("random_colour", [1, -1])
def test_one_colour_random(hc, st, random_colour):
    net = make_net(*NETS[0])
    white, black = (None, net) if random_colour == 1 else (net, None)
    out = host_rollout(hc, st, white, black)
    J = replay(hc, st, out, white, black)
    judge(J, f"random colour {random_colour}")
    assert J["random"] > 5000 and J["greedy"] > 5000


def test_nan_b2_picks_the_first_live_row(hc, st):
    """Every non-terminal row's value is NaN: the first NaN wins, whatever the
    terminal rows' outcomes (torch.max / torch.min's rule, aft_pick_row's)."""
    net = make_net(*NETS[0])
    with torch.no_grad():
        net.l2.bias.fill_(float("nan"))
    out = host_rollout(hc, st, net, net, plies=1)
    board, off, ft, player, _, _ = st
    ref = enumerate_turns(board, off, ft, player, out["dice"][0])
    seen = 0
    for e in range(board.shape[0]):
        r0, r1 = int(ref["offsets"][e]), int(ref["offsets"][e + 1])
        live = np.nonzero(ref["reward"][r0:r1] == 0)[0]
        if len(live):
            seen += 1
            assert out["row"][0, e] == live[0] and np.isnan(out["value"][0, e])
            assert np.array_equal(out["play"][0, e], ref["play"][r0 + live[0]])
    assert seen > 2000


@pytest.mark.parametrize("room,least", [(8, 0.4), (1, 0.9)])
def test_a_small_first_tier_gives_the_same_bits(hc, st, room, least):
    """room = 8: about half of the turns have a level of more than 8 nodes
    (49.7 % of this run's plies), room = 1: every turn with a choice; they
    outgrow the first tier and walk again at kTurnAftMax -- the same bits as
    room = 256."""
    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    a = host_rollout(hc, st, white, black)
    b = host_rollout(hc, st, white, black, room=room)
    share = b["tier"].mean()
    print(f"second tier at room {room}: {share:.1%} of plies; at room {ROOM}: {a['tier'].mean():.3%}")
    assert share > least and a["tier"].mean() < 0.01
    for k in ("dice", "play", "reward", "terminated", "truncated", "words", "rows", "row", "front", "mdice"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["value"].view(np.uint32), b["value"].view(np.uint32))
    for k, v in a["final"].items():
        assert np.array_equal(v, b["final"][k]), k
