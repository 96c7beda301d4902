"""The two-ply lookahead (narde_afterstates_lookahead: k_aft_fill_rec and
k_aft_look) on the CPU, through a test-only host build
that runs the kernels' shared functions serially
(tests/hostcheck/hostcheck_lookahead.cpp), against the reference pipeline of
tests/lookahead_ref.py built on reference_afterstates over the C oracle.

Tolerance: TOL_FACTOR (8) x E, E = max |pipeline in torch float32 - in
float64| on the same rows, floored at one float32 ulp of the largest
magnitude compared -- the reference's own rounding, never the code under
test's.  Terminal rows are exact.

The same inputs test the pass claim: on a (row, roll) with no reply, does
the step with actions (0, 0) -- the C oracle's or_step, which narde_step is
pinned to, and env_step, which k_step runs -- leave board and off counts
unchanged and the mover flipped?  Not always: code 0 is the bear-off from
point 0, and where every play that starts with it needs a second move no
code can express, the step bears that checker off and no row says so.  So
the step's own result is the definition (include/narde.h), the reference
takes it from the oracle, and the test asserts that both kinds occur.
(The kernel evaluates the 36 / 30 ordered rolls, so it does not rely on
(a, b) and (b, a) leaving the same afterstates; they do not: see
test_roll_order_matters.)
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT
from test_afterstates_cpu import golden_states, reference_afterstates

torch = pytest.importorskip("torch")

import lookahead_ref as LR  # noqa: E402
from test_value_cpu import TOL_FACTOR, make_net  # noqa: E402

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
# (hidden, g_hid, g_out, seed): the issue's sizes
NETS = [(80, "sigmoid", "sigmoid", 1), (1, "relu", "none", 3), (65, "relu", "tanh", 4), (128, "tanh", "none", 2)]
STRIDE = 13  # of golden_states(): 308 states
FUZZ = 60


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_lookahead.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_lookahead.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    lib.hc_lookahead.restype = ctypes.c_int64
    return lib


def lookahead_states():
    from fuzz_positions import random_positions

    g = [np.asarray(a)[::STRIDE] for a in golden_states()]
    board, off, ft, player, rng = random_positions(FUZZ, 17)
    dice = rng.integers(1, 7, (FUZZ, 2)).astype(np.uint8)
    return tuple(np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(g, (board, off, ft, player, dice)))


def reference_case(st, dice_mode="all36"):
    """The first-ply rows, their records, and per roll the replies of the
    non-terminal rows, all over the C oracle."""
    ref = reference_afterstates(*st)
    e = ref["row_env"]
    # the rows' records: the step itself (first_turn as narde_step leaves it)
    stp = O.step(st[0][e], st[1][e], st[2][e], st[3][e], st[4][e], ref["codes"], with_lists=False)
    assert np.array_equal(stp["board"], ref["board"]) and np.array_equal(stp["player"], ref["player"])
    live = ref["reward"] == 0
    rec = tuple(np.ascontiguousarray(stp[k][live]) for k in ("board", "off", "first_turn", "player"))
    n = int(live.sum())
    replies = []
    for a, b in LR.rolls_of(dice_mode):
        d = np.tile(np.array([a, b], np.uint8), (n, 1))
        rep = reference_afterstates(*rec, d)
        # no reply: what the step with the codes (0, 0) leaves
        ps = O.step(*rec, d, np.zeros((n, 2), np.int16), with_lists=False)
        rep.update(pass_feat=O.tesauro198(ps["board"], ps["off"], ps["player"]), pass_reward=ps["reward"],
                   pass_player=ps["player"], pass_board=ps["board"], pass_off=ps["off"])
        replies.append(rep)
    return dict(ref=ref, live=live, rec=rec, replies=replies, rolls=LR.rolls_of(dice_mode), ft=stp["first_turn"])


@pytest.fixture(scope="module")
def case():
    st = lookahead_states()
    return st, reference_case(st)


def host_lookahead(hc, st, net, cap=None, dice_mode=0):
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    n = st[0].shape[0]
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft, player, dice = c(st[0], np.int8), c(st[1], np.uint8), c(st[2], np.uint8), c(st[3], np.int8), c(st[4], np.uint8)
    w1t = c(net.l1.weight.detach().numpy().T, np.float32)
    b1, w2, b2 = (c(a.detach().numpy().reshape(-1), np.float32) for a in (net.l1.bias, net.l2.weight, net.l2.bias))
    offsets = np.zeros(n + 1, np.int32)

    def run(cap):
        o = dict(codes=np.zeros((cap, 2), np.int16), reward=np.zeros(cap, np.int8), value=np.full(cap, np.nan, np.float32),
                 board=np.zeros((cap, 24), np.int8), off=np.zeros((cap, 2), np.uint8), ft=np.zeros((cap, 2), np.uint8),
                 player=np.zeros(cap, np.int8), replies=np.zeros((cap, 36), np.int16),
                 terminal=np.zeros((cap, 36), np.uint8), best=np.zeros((cap, 36), np.float32))
        total = hc.hc_lookahead(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice), ctypes.c_int64(cap),
                                dice_mode, P(w1t), ctypes.c_int64(w1t.shape[1]), P(b1), P(w2), P(b2), net.hidden,
                                HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act], P(offsets),
                                *(P(o[k]) for k in ("codes", "reward", "value", "board", "off", "ft", "player",
                                                    "replies", "terminal", "best")))
        return total, o

    if cap is None:
        cap, _ = run(0)
    total, o = run(int(cap))
    return dict(o, offsets=offsets.copy(), total=total)


def test_inputs_hold_the_cases_that_matter(case):
    st, c = case
    ref, live = c["ref"], c["live"]
    assert 300 <= st[0].shape[0] <= 400
    term_player = ref["player"][~live]
    assert (term_player == 1).any() and (term_player == -1).any()  # a terminal first-ply row of each colour
    assert (np.diff(ref["offsets"]) == 0).any()  # an env with no row
    cnt = np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1)
    assert (cnt == 0).any()  # a (row, roll) with no reply
    assert any((r["reward"] != 0).any() for r in c["replies"])  # a terminal reply
    assert (c["rec"][3] == 1).any() and (c["rec"][3] == -1).any()  # both colours reply
    assert max(int(r["plays"].max()) for r in c["replies"]) > 128  # a reply's plays span three chunks of the wave
    assert cnt.max() >= 64


def test_what_the_step_leaves_where_there_is_no_reply(hc, case):
    """Every (row, roll) with no reply, the step with (0, 0): the oracle's and
    env_step's results agree, the game never ends there, and the result is the
    position with the mover flipped except where point 0's checker is borne
    off."""
    st, c = case
    board, off, ft, player = c["rec"]
    passes = moved = 0
    for (a, b), rep in zip(c["rolls"], c["replies"]):
        idx = np.nonzero(np.diff(rep["offsets"]) == 0)[0]
        if not len(idx):
            continue
        d = np.tile(np.array([a, b], np.uint8), (len(idx), 1))
        pb, po, pp = rep["pass_board"][idx], rep["pass_off"][idx], rep["pass_player"][idx]
        assert np.array_equal(pp, -player[idx]) and not rep["pass_reward"][idx].any()
        # env_step, the function k_step runs
        hb, ho, hf, hp = (np.ascontiguousarray(x[idx]).copy() for x in (board, off, ft, player))
        rew = np.full(len(idx), 9, np.int8)
        hc.hc_lookahead_pass(ctypes.c_int64(len(idx)), P(hb), P(ho), P(hf), P(hp), P(d), P(rew))
        assert np.array_equal(hb, pb) and np.array_equal(ho, po) and np.array_equal(hp, pp) and not rew.any()
        same = (pb == board[idx]).all(1) & (po == off[idx]).all(1)
        passes += int(same.sum())
        moved += int((~same).sum())
        # the exception: the mover's checkers on its point 0 borne off, nothing else
        for q in np.nonzero(~same)[0]:
            w = player[idx][q] == 1
            gone = int(po[q][0 if w else 1]) - int(off[idx][q][0 if w else 1])
            diff = np.nonzero(pb[q] != board[idx][q])[0]
            assert gone in (1, 2) and diff.tolist() == [0 if w else 12]
            assert abs(int(board[idx][q][diff[0]])) - abs(int(pb[q][diff[0]])) == gone
    print(f"no-reply (row, roll) pairs: {passes} passes, {moved} where the step bears point 0 off")
    assert passes > 0 and moved > 0


def test_roll_order_matters(case):
    """(a, b) and (b, a) do not always leave the same set of (board, off,
    reward) afterstates -- why the kernel takes the ordered rolls."""
    st, c = case
    rolls = c["rolls"]
    differ = 0
    for i, (a, b) in enumerate(rolls):
        if a >= b:
            continue
        x, y = c["replies"][i], c["replies"][rolls.index((b, a))]
        for r in range(len(c["rec"][3])):
            key = lambda w: {w["board"][q].tobytes() + w["off"][q].tobytes() + w["reward"][q].tobytes()  # noqa: E731
                             for q in range(w["offsets"][r], w["offsets"][r + 1])}
            differ += key(x) != key(y)
    print(f"(row, unordered roll) pairs whose two orders leave different sets: {differ}")
    assert differ > 0


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_lookahead_through_the_shared_functions(hc, case, spec):
    st, c = case
    ref, live = c["ref"], c["live"]
    net = make_net(*spec)
    got = host_lookahead(hc, st, net)
    # the rows are narde_afterstates': order, codes, reward, and their records
    assert np.array_equal(got["offsets"], ref["offsets"]) and got["total"] == len(live)
    for k in ("codes", "reward", "board", "off", "player"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["ft"], c["ft"])
    cnt = np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1)
    cols = [6 * (a - 1) + (b - 1) for a, b in c["rolls"]]
    assert np.array_equal(got["replies"][live][:, cols], cnt) and (got["replies"][~live] == -1).all()
    ends = np.zeros(cnt.shape, np.uint8)  # a reply of the (row, roll) ends the game
    for q, r in enumerate(c["replies"]):
        ends[np.repeat(np.arange(cnt.shape[0]), cnt[:, q])[r["reward"] != 0], q] = 1
    assert np.array_equal(got["terminal"][live][:, cols], ends) and ends.any()
    want, w32, m64 = LR.two_ply(net, c["replies"], c["rec"][3] == -1)
    E = LR.error_bound(w32, want)
    tol = TOL_FACTOR * E
    assert np.ptp(want) > 1e3 * tol  # the values differ: a wrong reply would show
    err = float(np.abs(got["value"][live].astype(np.float64) - want).max())
    errm = float(np.abs(got["best"][live][:, cols].astype(np.float64) - m64).max())
    print(f"{spec[:3]}: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E; per roll {errm:.3e} = {errm / E:.2f} E")
    assert err <= tol, (err, tol)
    # terminal rows: the outcome, exactly
    r = ref["reward"][~live].astype(np.float32)
    assert np.array_equal(got["value"][~live], np.where(ref["player"][~live] == -1, -r, r))
    # and the values are not the one-ply ones
    one = LR.copy.deepcopy(net).double()(torch.from_numpy(ref["feat"][live]).double()).detach().numpy().reshape(-1)
    assert np.abs(one - want).max() > 1e3 * tol


def test_nodoubles_takes_the_30_roll_mean(hc, case):
    st, c = case
    net = make_net(*NETS[0])
    got = host_lookahead(hc, st, net, dice_mode=1)
    keep = [i for i, (a, b) in enumerate(c["rolls"]) if a != b]
    assert len(keep) == 30
    want, w32, _ = LR.two_ply(net, [c["replies"][i] for i in keep], c["rec"][3] == -1)
    E = LR.error_bound(w32, want)
    live = c["live"]
    err = float(np.abs(got["value"][live].astype(np.float64) - want).max())
    print(f"nodoubles: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E")
    assert err <= TOL_FACTOR * E
    w36, _, _ = LR.two_ply(net, c["replies"], c["rec"][3] == -1)
    assert np.abs(w36 - want).max() > 1e3 * TOL_FACTOR * E  # not the 36-roll mean
    doubles = [6 * k + k for k in range(6)]
    assert (got["replies"][live][:, doubles] == -1).all()


def test_cap_clamps_rows_not_offsets(hc, case):
    st, c = case
    net = make_net(*NETS[0])
    full = host_lookahead(hc, st, net)
    cap = full["total"] // 2
    got = host_lookahead(hc, st, net, cap=cap)
    assert got["total"] == full["total"] and np.array_equal(got["offsets"], full["offsets"])
    assert np.array_equal(got["value"].view(np.uint32), full["value"][:cap].view(np.uint32))
    assert np.array_equal(got["codes"], full["codes"][:cap])
