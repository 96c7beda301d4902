"""The FULL4 two-ply lookahead (narde_turn_afterstates_lookahead: the record
fills, k_turn_look, k_turn_look_mean) on the CPU,
through a test-only host build that runs the kernels' shared functions
serially (tests/hostcheck/hostcheck_turn_lookahead.cpp), against the reference
pipeline of tests/turn_lookahead_ref.py built on enumerate_turns over the C
oracle.

Tolerance: TOL_FACTOR (8) x E, E = max |pipeline in torch float32 - in
float64| on the same rows, floored at one float32 ulp of the largest
magnitude compared -- the reference's own rounding, never the code under
test's.  Terminal rows are exact, and so are the rows' records (first-turn
flags included), every (row, roll) reply count and the pass position.

The same inputs settle the two claims include/narde.h states: a pass (row,
roll) leaves the row's position with the mover flipped and nothing else
changed, always; and (a, b) and (b, a) give the same reply rows in the same
order, so the kernel evaluates the 21 unordered rolls.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, golden

torch = pytest.importorskip("torch")

import turn_afterstates_ref as R  # noqa: E402
import turn_lookahead_ref as TL  # noqa: E402
from test_value_cpu import TOL_FACTOR, make_net  # noqa: E402

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
# (hidden, g_hid, g_out, seed): the issue's sizes
NETS = [(80, "sigmoid", "sigmoid", 1), (1, "relu", "none", 3), (65, "relu", "tanh", 4), (128, "tanh", "none", 2)]
GOLDEN_STRIDE = 150  # of tests/golden/full4.npz: 111 states
SPREAD_SEED = 711  # spread_replier_states(16, .): 142 rows, 64 (row, roll) pairs above 256 reply rows on 15 rows


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_turn_lookahead.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_turn_lookahead.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    lib.hc_turn_lookahead.restype = ctypes.c_int64
    return lib


def lookahead_states():
    g = {k: np.asarray(v)[::GOLDEN_STRIDE] for k, v in R.golden_states(golden("full4.npz")).items()}
    return R.concat(g, R.selfplay_states(n=8, plies=120, every=12, seed=3), R.edge_states(), R.start_states())


@pytest.fixture(scope="module")
def case():
    st = lookahead_states()
    return st, TL.reference_case(st, both_orders=True)


def host_lookahead(hc, st, net, cap=None, dice_mode=0):
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft = c(st["board"], np.int8), c(st["off"], np.uint8), c(st["ft"], np.uint8)
    player, dice = c(st["player"], np.int8), c(st["dice"], np.uint8)
    n = board.shape[0]
    w1t = c(net.l1.weight.detach().numpy().T, np.float32)
    b1, w2, b2 = (c(a.detach().numpy().reshape(-1), np.float32) for a in (net.l1.bias, net.l2.weight, net.l2.bias))
    offsets = np.zeros(n + 1, np.int32)

    def run(cap):
        o = dict(play=np.full((cap, 4, 2), 99, np.int8), reward=np.zeros(cap, np.int8),
                 value=np.full(cap, np.nan, np.float32), board=np.zeros((cap, 24), np.int8),
                 off=np.zeros((cap, 2), np.uint8), ft=np.zeros((cap, 2), np.uint8), player=np.zeros(cap, np.int8),
                 replies=np.zeros((cap, 21), np.int32), front=np.zeros((cap, 21), np.int32),
                 terminal=np.zeros((cap, 21), np.uint8), best=np.zeros((cap, 21), np.float32))
        total = hc.hc_turn_lookahead(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice), ctypes.c_int64(cap),
                                     dice_mode, P(w1t), ctypes.c_int64(w1t.shape[1]), P(b1), P(w2), P(b2), net.hidden,
                                     HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act], P(offsets),
                                     *(P(o[k]) for k in ("play", "reward", "value", "board", "off", "ft", "player",
                                                         "replies", "front", "terminal", "best")))
        return total, o

    if cap is None:
        cap, _ = run(0)
    total, o = run(int(cap))
    return dict(o, offsets=offsets.copy(), total=total)


def reply_counts(c):
    return np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1)


def test_inputs_hold_the_cases_that_matter(case):
    st, c = case
    ref, live = c["ref"], c["live"]
    assert 200 <= len(st["player"]) <= 300
    term_player = ref["player"][~live]
    assert (term_player == 1).any() and (term_player == -1).any()  # a terminal first-ply row of each colour
    cnt = reply_counts(c)
    assert (cnt == 0).any()  # pass (row, roll) pairs
    assert any((r["reward"] != 0).any() for r in c["replies"])  # a terminal reply
    assert (c["rec"][3] == 1).any() and (c["rec"][3] == -1).any()  # both colours reply
    # a first-turn replier on 3-3, 4-4 or 6-6 with two head moves in a reply
    two_heads = 0
    for k, r in zip(c["ks"], c["replies"]):
        if TL.ROLLS[k] in ((3, 3), (4, 4), (6, 6)):
            row = np.repeat(np.arange(len(c["rec"][3])), np.diff(r["offsets"]))
            replier_ft = c["rec"][2][row, np.where(c["rec"][3][row] == 1, 0, 1)]
            heads = (r["play"][:, :, 0] == 23).sum(1)
            assert (heads[replier_ft == 0] <= 1).all()
            two_heads += int(((heads == 2) & (replier_ft == 1)).sum())
    assert two_heads > 0
    # a two-different-dice reply with M = 1 on the higher die
    m1_high = 0
    for k, r in zip(c["ks"], c["replies"]):
        a, b = TL.ROLLS[k]
        if a != b:
            row = np.repeat(np.arange(len(c["rec"][3])), np.diff(r["offsets"]))
            m1_high += int(((r["max_dice"][row] == 1) & (r["play"][:, 0, 1] == b)).sum())
    assert m1_high > 0
    assert cnt.max() > 64  # a reply whose final level spans more than one 64-node chunk


def test_a_pass_leaves_the_position_with_the_mover_flipped(case):
    """Every (row, roll) with M = 0: the oracle's step with an all -1 play
    leaves board, off counts and both first-turn flags as they are, ends no
    game and flips the mover -- no exception (include/narde.h states the
    count)."""
    st, c = case
    board, off, ft, player = c["rec"]
    passes = 0
    for rep in c["replies"]:
        idx = np.nonzero(np.diff(rep["offsets"]) == 0)[0]
        assert (rep["pass_max_dice"][idx] == 0).all() and (rep["max_dice"][idx] == 0).all()
        assert np.array_equal(rep["pass_board"][idx], board[idx]) and np.array_equal(rep["pass_off"][idx], off[idx])
        assert np.array_equal(rep["pass_ft"][idx], ft[idx])
        assert np.array_equal(rep["pass_player"][idx], -player[idx]) and not rep["pass_reward"][idx].any()
        passes += len(idx)
    print(f"pass (row, roll) pairs: {passes}, every one the position with the mover flipped")
    assert passes > 0


def test_roll_order_does_not_matter(case):
    """(a, b) and (b, a): the same reply rows in the same order on the whole
    input set -- why the kernel takes the unordered rolls."""
    st, c = case
    assert len(c["swapped"]) == 15
    for k, y in c["swapped"]:
        x = c["replies"][c["ks"].index(k)]
        for key in ("offsets", "play", "board", "off", "player", "reward", "max_dice"):
            assert np.array_equal(x[key], y[key]), (TL.ROLLS[k], key)


def compare_with_reference(hc, st, c, spec):
    """The host build on st against the reference case c, net spec: rows,
    records, reply counts, terminal marks, values within 8 E.  Returns (got,
    want, tol)."""
    ref, live = c["ref"], c["live"]
    net = make_net(*spec)
    got = host_lookahead(hc, st, net)
    # the rows are narde_turn_afterstates': order, play, reward, and their records as the step leaves them
    assert np.array_equal(got["offsets"], ref["offsets"]) and got["total"] == len(live)
    for k in ("play", "reward", "board", "off", "player"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["ft"], c["ft"])
    mover = np.where(np.asarray(st["player"])[ref["row_env"]] == 1, 0, 1)
    assert not got["ft"][np.arange(len(mover)), mover].any()  # the side that moved has its flag cleared
    cnt = reply_counts(c)
    assert np.array_equal(got["replies"][live][:, c["ks"]], cnt) and (got["replies"][~live] == -1).all()
    ends = np.zeros(cnt.shape, np.uint8)  # a reply of the (row, roll) ends the game
    for q, r in enumerate(c["replies"]):
        ends[np.repeat(np.arange(cnt.shape[0]), cnt[:, q])[r["reward"] != 0], q] = 1
    assert np.array_equal(got["terminal"][live][:, c["ks"]], ends)
    want, w32, m64 = TL.two_ply_weighted(net, c["replies"], c["ks"], c["rec"][3] == -1)
    E = TL.error_bound(w32, want)
    tol = TOL_FACTOR * E
    assert np.ptp(want) > 1e3 * tol  # the values differ: a wrong reply would show
    err = float(np.abs(got["value"][live].astype(np.float64) - want).max())
    errm = float(np.abs(got["best"][live][:, c["ks"]].astype(np.float64) - m64).max())
    print(f"{spec[:3]}: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E; per roll {errm:.3e} = {errm / E:.2f} E")
    assert err <= tol, (err, tol)
    assert errm <= tol, (errm, tol)
    # terminal rows: the outcome, exactly
    r = ref["reward"][~live].astype(np.float32)
    assert np.array_equal(got["value"][~live], np.where(ref["player"][~live] == -1, -r, r))
    # and the values are not the one-ply ones
    one = TL.LR.copy.deepcopy(net).double()(torch.from_numpy(ref["feat"][live]).double()).detach().numpy().reshape(-1)
    assert np.abs(one - want).max() > 1e3 * tol
    return got, ends


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_lookahead_through_the_shared_functions(hc, case, spec):
    st, c = case
    got, ends = compare_with_reference(hc, st, c, spec)
    assert ends.any()


def test_spread_repliers_off_selfplay(hc):
    """Run-heavy boards with the piled side to move and the spread side
    replying (tests/fuzz_positions.py): reply walks that outgrow the fast
    frontier by the dozen, several rolls of one row among them."""
    from fuzz_positions import spread_replier_states

    st = spread_replier_states(16, SPREAD_SEED)
    c = TL.reference_case(st)
    cnt = reply_counts(c)
    big = cnt > 256
    print(f"rows {len(c['live'])}, reply rows {int(cnt.sum())}, (row, roll) pairs above 256 reply rows {int(big.sum())}, "
          f"rows with two or more {int((big.sum(1) >= 2).sum())}")
    assert big.sum() >= 30 and (big.sum(1) >= 2).any()
    got, _ = compare_with_reference(hc, st, c, NETS[0])
    # a (row, roll) with more than 256 replies has a level above the fast frontier's 256 nodes
    assert (got["front"][c["live"]][:, c["ks"]][big] > 256).all()


def test_nodoubles_takes_the_15_roll_mean(hc, case):
    st, c = case
    net = make_net(*NETS[0])
    got = host_lookahead(hc, st, net, dice_mode=1)
    keep = [i for i, k in enumerate(c["ks"]) if TL.ROLLS[k][0] != TL.ROLLS[k][1]]
    assert len(keep) == 15
    black = c["rec"][3] == -1
    want, w32, _ = TL.two_ply_weighted(net, [c["replies"][i] for i in keep], [c["ks"][i] for i in keep], black)
    E = TL.error_bound(w32, want)
    live = c["live"]
    err = float(np.abs(got["value"][live].astype(np.float64) - want).max())
    print(f"nodoubles: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E")
    assert err <= TOL_FACTOR * E
    w36, _, _ = TL.two_ply_weighted(net, c["replies"], c["ks"], black)
    assert np.abs(w36 - want).max() > 1e3 * TOL_FACTOR * E  # not the 36-roll mean
    doubles = [k for k, (a, b) in enumerate(TL.ROLLS) if a == b]
    assert (got["replies"][live][:, doubles] == -1).all()


def test_cap_clamps_rows_not_offsets(hc, case):
    st, c = case
    net = make_net(*NETS[0])
    full = host_lookahead(hc, st, net)
    cap = full["total"] // 2
    got = host_lookahead(hc, st, net, cap=cap)
    assert got["total"] == full["total"] and np.array_equal(got["offsets"], full["offsets"])
    assert np.array_equal(got["value"].view(np.uint32), full["value"][:cap].view(np.uint32))
    assert np.array_equal(got["play"], full["play"][:cap])


@pytest.mark.parametrize("points,lo,hi", [(TL.TIER_SLAB_POINTS, 2049, R.BIG_ROWS), (TL.TIER_LDS_POINTS, 257, 2048)],
                         ids=["slab", "lds"])
def test_overflow_tier_positions(hc, points, lo, hi):
    """The parents whose rows' reply walks leave the 256-node fast path: one
    with a level above 2,048 nodes (the slab tier: big_state() handed to
    white, who replies with 1-1), one whose largest level lies in
    257..2,048 (the LDS tier).  The counts are the reference enumerator's;
    the walk's largest level the host build's."""
    st = TL.tier_state(points)
    c = TL.reference_case(st)
    cnt = reply_counts(c)
    net = make_net(17, "tanh", "none", 5)
    got = host_lookahead(hc, st, net)
    assert np.array_equal(got["replies"][:, c["ks"]], cnt) and c["live"].all()
    if hi == R.BIG_ROWS:  # black's one row hands big_state() to white: 2,065 rows at 1-1
        assert len(c["live"]) == 1 and cnt[0, 0] == R.BIG_ROWS
        assert np.array_equal(c["rec"][0][0], R.big_state()["board"]) and c["rec"][3][0] == 1
    front = int(got["front"].max())
    assert lo <= cnt.max() <= hi and lo <= front and (front <= hi or hi == R.BIG_ROWS)
    want, w32, m64 = TL.two_ply_weighted(net, c["replies"], c["ks"], c["rec"][3] == -1)
    E = TL.error_bound(w32, want)
    err = float(np.abs(got["value"].astype(np.float64) - want).max())
    print(f"tier {lo}..{hi}: rows {len(c['live'])}, largest level {front}, E = {E:.3e}, max error = {err / E:.2f} E")
    assert err <= TOL_FACTOR * E
