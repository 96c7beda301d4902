"""The Monte-Carlo playouts (narde_value_playout / narde_turn_value_playout:
k_value_playout, k_turn_value_playout) on the CPU,
through a test-only host build that runs the kernels' shared functions
serially (tests/hostcheck/hostcheck_value_playout.cpp).

The oracle is the host rollout that existed before (hc_value_rollout /
hc_turn_value_rollout, themselves replayed over the C oracle by
tests/test_value_rollout_cpu.py and tests/test_turn_value_rollout_cpu.py): root
i copied to env index q = i * trials + j of a run with the same seed, env0 =
id_base, the roots' ply counter and max_steps = 0.  Trial (i, j) must equal
that env's first terminal ply exactly: finished or not, the length, the
outcome's sign and size.

leaf: against the net in torch float64 on O.tesauro198 of the position the
oracle's env holds after max_plies plies, within TOL_FACTOR x E
(tests/test_value_cpu.py), E = max |torch float32 - torch float64| on the same
rows, floored at one float32 ulp of the largest value -- the reference's own
rounding, computed from the reference alone.
"""
import copy
import ctypes
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT

torch = pytest.importorskip("torch")

from test_value_cpu import TOL_FACTOR, make_net  # noqa: E402
from test_value_rollout_cpu import BLACK, NETS, SEED, P, endgames, net_in, ply_words, start_states  # noqa: E402

ROOM = 256
PLIES = 6  # leaves most non-endgame trials unfinished
FULL = {"ref2": 0, "full4": 1}


def _lib(name):
    path = os.path.join(ROOT, "tests", "hostcheck", "build", name)
    if not os.path.exists(path):
        pytest.fail(f"tests/hostcheck/build/{name} is missing: run __graft_entry__.build()")
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def hcp():
    return _lib("libhostcheck_value_playout.so")


@pytest.fixture(scope="module")
def hc_roll():
    return {"ref2": _lib("libhostcheck_value_rollout.so"), "full4": _lib("libhostcheck_turn_value_rollout.so")}


def late_races():
    """Four positions two or three turns from the end: every checker left is
    in its owner's home (white's points 0..5, black's 12..17), 11 or 12 off a
    side."""
    board = np.zeros((4, 24), np.int8)
    off = np.zeros((4, 2), np.uint8)
    board[0, [1, 3, 4]], board[0, [13, 15]], off[0] = 1, (-1, -2), (12, 12)
    board[1, [0, 2, 5]], board[1, [12, 14, 17]], off[1] = (2, 1, 1), (-1, -1, -1), (11, 12)
    board[2, [2, 3]], board[2, [13, 16, 17]], off[2] = (1, 2), (-2, -1, -1), (12, 11)
    board[3, [0, 1, 4, 5]], board[3, [12, 13]], off[3] = 1, (-2, -1), (11, 12)
    return board, off, np.zeros((4, 2), np.uint8), np.array([1, -1, -1, 1], np.int8)


@pytest.fixture(scope="module")
def roots():
    """start_states()' positions (golden states, fuzz positions, the four endgames)"""
    return tuple(a.copy() for a in start_states()[:4])


def some(state, step):
    """every step-th root and the last four (the endgames)"""
    n = state[0].shape[0]
    idx = np.unique(np.concatenate([np.arange(0, n - 4, step), np.arange(n - 4, n)]))
    return tuple(np.ascontiguousarray(a[idx]) for a in state)


def host_playout(hcp, rules, state, t, trials, max_plies, white, black, seed=SEED, id_base=0, common=False,
                 dice_mode=0, room=ROOM):
    board, off, ft, player = (np.ascontiguousarray(a) for a in state)
    n = board.shape[0]
    keep = []
    o = dict(records=np.zeros((n, 8), np.uint32), sums=np.full((n, 4), -1, np.int32),
             outcome=np.full((n, trials), 99, np.int8), length=np.zeros((n, trials), np.int32),
             leaf=np.zeros((n, trials), np.float32))
    w, b = net_in(white, keep), net_in(black, keep)
    hcp.hc_value_playout(FULL[rules], room, ctypes.c_int64(n), P(board), P(off), P(ft), P(player), ctypes.c_uint32(t),
                         trials, max_plies, ctypes.byref(w), ctypes.byref(b), ctypes.c_uint64(seed),
                         ctypes.c_int64(id_base), int(common), dice_mode,
                         *(P(o[k]) for k in ("records", "sums", "outcome", "length", "leaf")))
    return o


def oracle_rollout(hc_roll, rules, state, t, trials, max_plies, white, black, seed=SEED, id_base=0, dice_mode=0):
    """The existing host rollout on every root `trials` times over: per trial
    done, outcome, length, and the position after max_plies plies."""
    board, off, ft, player = (np.ascontiguousarray(np.repeat(a, trials, axis=0)) for a in state)
    B = board.shape[0]
    n = B // trials
    elapsed, tt, stats = np.zeros(B, np.uint16), np.full(B, t, np.uint32), np.zeros((B, 3), np.int32)
    keep = []
    w, b = net_in(white, keep), net_in(black, keep)
    z = lambda shape, dt: np.zeros((max_plies, B) + shape, dt)  # noqa: E731
    reward, term, trunc = z((), np.int32), z((), np.uint8), z((), np.uint8)
    movers = np.zeros((max_plies, B), np.int8)
    common = [ctypes.c_int64(B), P(board), P(off), P(ft), P(player), P(elapsed), P(tt), P(stats),
              ctypes.c_int64(id_base), ctypes.c_uint64(seed), dice_mode, 0]
    tail = [ctypes.byref(w), ctypes.byref(b), 0, ctypes.c_float(0.0), ctypes.c_uint64(0), ctypes.c_int64(0)]
    # one ply a call, so that each ply's mover is known (the rollout's outputs do not name it)
    for k in range(max_plies):
        movers[k] = player
        one = [P(a[k]) for a in (reward, term, trunc)]
        if rules == "full4":
            assert dice_mode == 0
            hc_roll[rules].hc_turn_value_rollout(*common, 1, ROOM, *tail, P(np.zeros((B, 2), np.uint8)),
                                                 P(np.zeros((B, 4, 2), np.int8)), P(np.zeros(B, np.float32)), *one,
                                                 P(np.zeros((B, 4), np.uint32)), P(np.zeros(B, np.int32)),
                                                 P(np.zeros(B, np.int32)), P(np.zeros(B, np.uint8)),
                                                 P(np.zeros(B, np.uint8)), P(np.zeros(B, np.int32)),
                                                 P(np.zeros(B, np.int32)))
        else:
            hc_roll[rules].hc_value_rollout(*common, 1, *tail, P(np.zeros((B, 2), np.uint8)),
                                            P(np.zeros((B, 2), np.int16)), P(np.zeros(B, np.float32)), *one,
                                            P(np.zeros((B, 4), np.uint32)), P(np.zeros(B, np.int32)),
                                            P(np.zeros(B, np.int32)), P(np.zeros(B, np.uint8)))
    assert not trunc.any()
    done = term.any(0)
    first = np.where(done, term.argmax(0), max_plies - 1)
    q = np.arange(B)
    outcome = np.where(done, movers[first, q].astype(np.int64) * reward[first, q], 0)
    o = dict(done=done.reshape(n, trials), outcome=outcome.reshape(n, trials).astype(np.int8),
             length=(first + 1).reshape(n, trials).astype(np.int32),
             feat=O.tesauro198(board, off, player).reshape(n, trials, 198), stop_player=player.reshape(n, trials))
    return o


def test_one_ply_a_call_is_the_rollouts_own_run(hc_roll, roots):
    """oracle_rollout() calls the host rollout a ply at a time (the Philox
    block is redrawn on every call's first ply from the env's own counter):
    the same rewards and flags as one call of all the plies."""
    from test_value_rollout_cpu import host_rollout

    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    st = some(roots, 5)
    n = st[0].shape[0]
    whole = host_rollout(hc_roll["ref2"], st + (np.zeros(n, np.uint16), np.full(n, 3, np.uint32)), white, black,
                         plies=PLIES, max_steps=0)
    want = oracle_rollout(hc_roll, "ref2", st, 3, 1, PLIES, white, black, id_base=5)  # (host_rollout's ENV0)
    term = whole["terminated"] != 0
    assert np.array_equal(want["done"][:, 0], term.any(0))
    fin = term.any(0)
    assert np.array_equal(want["length"][fin, 0], term.argmax(0)[fin] + 1)


def compare(got, want, what):
    assert np.array_equal(got["outcome"] != 0, want["done"]), f"{what}: finished"
    assert np.array_equal(got["length"], want["length"]), f"{what}: length"
    assert np.array_equal(got["outcome"], want["outcome"]), f"{what}: outcome"
    oc = got["outcome"].astype(np.int64)
    sums = np.stack([(oc != 0).sum(1), oc.sum(1), (oc * oc).sum(1), got["length"].sum(1)], 1)
    assert np.array_equal(got["sums"], sums.astype(np.int32)), f"{what}: sums"


def check_leaf(got, want, white, black, what):
    leaf, done = got["leaf"], want["done"]
    assert np.array_equal(np.isnan(leaf), done), f"{what}: leaf is NaN exactly where the trial finished"
    for colour, own, other in ((1, white, black), (-1, black, white)):
        net = own if own is not None else other
        sel = ~done & (want["stop_player"] == colour)
        if not sel.any():
            continue
        x = torch.from_numpy(np.ascontiguousarray(want["feat"][sel]))
        with torch.no_grad():
            v32 = net(x).double().numpy().reshape(-1)
            v64 = copy.deepcopy(net).double()(x.double()).numpy().reshape(-1)
        E = max(float(np.abs(v32 - v64).max()), float(np.spacing(np.float32(max(np.abs(v64).max(), 1e-30)))))
        err = float(np.abs(leaf[sel].astype(np.float64) - v64).max())
        print(f"{what}: colour {colour}: {int(sel.sum())} leaves, max |leaf - ref| = {err:.3e}, E = {E:.3e}")
        assert err <= TOL_FACTOR * E, (what, colour, err, E)


# (spec, trials, id_base, black): every H of NETS, both trial counts, both id bases, one colour random once
UNFINISHED = [(NETS[0], 5, 0, "net"), (NETS[1], 1, 1000, "net"), (NETS[2], 5, 1000, None), (NETS[3], 1, 0, "net")]


@pytest.mark.parametrize("rules", list(FULL))
@pytest.mark.parametrize("spec,trials,id_base,black", UNFINISHED,
                         ids=[f"H{s[0]}-trials{t}-id{i}-{'random-black' if b is None else 'two-nets'}"
                              for s, t, i, b in UNFINISHED])
def test_trials_are_the_rollouts_first_terminal_plies(hcp, hc_roll, roots, rules, spec, trials, id_base, black):
    white = make_net(*spec)
    black = None if black is None else make_net(*BLACK[spec[0]])
    st = some(roots, 1 if trials == 1 else 3)
    t = 3
    want = oracle_rollout(hc_roll, rules, st, t, trials, PLIES, white, black, id_base=id_base)
    unfinished = 1.0 - want["done"].mean()
    print(f"{rules} H {spec[0]}: {st[0].shape[0]} roots x {trials} trials, {unfinished:.0%} unfinished by the oracle")
    assert unfinished >= 0.25  # the leaf path is exercised
    assert want["done"][-4:].all()  # and the endgames finish
    got = host_playout(hcp, rules, st, t, trials, PLIES, white, black, id_base=id_base)
    compare(got, want, f"{rules} H {spec[0]}")
    check_leaf(got, want, white, black, f"{rules} H {spec[0]}")


@pytest.mark.parametrize("rules", list(FULL))
def test_a_finishing_case(hcp, hc_roll, rules):
    """The endgames and positions two or three turns from the end: the host
    rollout shows every trial finished within max_plies."""
    st = tuple(np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(late_races(), endgames()))
    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    trials, max_plies = 5, 40
    want = oracle_rollout(hc_roll, rules, st, 0, trials, max_plies, white, black, id_base=17)
    assert want["done"].all() and want["length"][:4].max() > 1 and want["length"].max() < max_plies
    got = host_playout(hcp, rules, st, 0, trials, max_plies, white, black, id_base=17)
    compare(got, want, rules)
    assert (got["sums"][:, 0] == trials).all() and np.isnan(got["leaf"]).all()


@pytest.mark.parametrize("rules", list(FULL))
def test_the_endgames_points_are_the_c_oracles(hcp, rules):
    """One ply from winning: any roll bears the last checker off.  O.step with
    the trial's own dice and the bear-off code gives the reward, 1 or 2; white's
    outcome is that, signed by the mover."""
    st = endgames()
    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    trials, t, id_base = 5, 2, 40
    got = host_playout(hcp, rules, st, t, trials, PLIES, white, black, id_base=id_base)
    assert (got["length"] == 1).all() and np.isnan(got["leaf"]).all()
    for i in range(4):
        for j in range(trials):
            k36 = (ply_words(t, id_base + i * trials + j)[0] * 36) >> 32
            dice = np.array([[k36 // 6 + 1, k36 % 6 + 1]], np.uint8)
            stp = O.step(st[0][i:i + 1], st[1][i:i + 1], st[2][i:i + 1], st[3][i:i + 1], dice,
                         np.zeros((1, 2), np.int16), with_lists=False)  # code 0: (0, 'off')
            assert stp["terminated"][0] == 1 and int(stp["reward"][0]) == (1, 2, 1, 2)[i]
            assert got["outcome"][i, j] == int(st[3][i]) * int(stp["reward"][0])
    assert np.array_equal(got["sums"], np.array([[5, 5, 5, 5], [5, 10, 20, 5], [5, -5, 5, 5], [5, -10, 20, 5]]))


@pytest.mark.parametrize("rules", list(FULL))
def test_common_dice_equals_the_single_root_calls(hcp, roots, rules):
    st = some(roots, 12)
    white, black = make_net(*NETS[3]), make_net(*BLACK[128])
    trials, t, id_base = 5, 1, 9
    many = host_playout(hcp, rules, st, t, trials, PLIES, white, black, id_base=id_base, common=True)
    plain = host_playout(hcp, rules, st, t, trials, PLIES, white, black, id_base=id_base)
    n = st[0].shape[0]
    for i in range(n):
        one = host_playout(hcp, rules, tuple(a[i:i + 1] for a in st), t, trials, PLIES, white, black, id_base=id_base)
        for k in ("sums", "outcome", "length"):
            assert np.array_equal(many[k][i:i + 1], one[k]), (i, k)
        assert np.array_equal(many["leaf"][i:i + 1].view(np.uint32), one["leaf"].view(np.uint32)), i
    assert not np.array_equal(many["leaf"][1:].view(np.uint32), plain["leaf"][1:].view(np.uint32))


def test_full4_bits_do_not_depend_on_the_first_tier(hcp, roots):
    """room = 8 sends most walks to the second tier: the same bits as room = 256."""
    from turn_afterstates_ref import big_state

    big = big_state()
    st = some(roots, 40)
    st = tuple(np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(
        st, (big["board"][None], big["off"][None], big["ft"][None], np.array([big["player"]], np.int8))))
    white, black = make_net(*NETS[0]), make_net(*BLACK[80])
    a = host_playout(hcp, "full4", st, 0, 2, PLIES, white, black, room=ROOM)
    b = host_playout(hcp, "full4", st, 0, 2, PLIES, white, black, room=8)
    for k in ("sums", "outcome", "length"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["leaf"].view(np.uint32), b["leaf"].view(np.uint32))


def test_records_are_set_states_packing(hcp, roots):
    """narde_state_records' records: the ply counter t in word 7, elapsed 0, and
    the position the rollout's own packing (record_from_board) gives."""
    st = some(roots, 7)
    got = host_playout(hcp, "ref2", st, 0x12345, 1, 1, make_net(*NETS[1]), None)
    rec = got["records"]
    assert (rec[:, 7] == 0x12345).all()
    assert np.array_equal((rec[:, 6] >> 10) & 1, (st[3] == -1).astype(np.uint32))
    other = host_playout(hcp, "ref2", st, 7, 1, 1, make_net(*NETS[1]), None)["records"]
    assert np.array_equal(rec[:, :7], other[:, :7]) and (other[:, 7] == 7).all()
