"""Afterstate expansion (narde_rules.h "afterstates": the per-play functions
of k_aft_count / k_aft_fill) on the CPU, through a test-only host build that
walks each env's plays serially (tests/hostcheck/hostcheck_afterstates.cpp),
against a restatement over the C oracle's primitives: the ordered plays of
narde_env.py:45-93, the expressibility filter, NardeEnv.step on the
surviving codes, the first of equal (board, off) kept, O.tesauro198 rows.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT, golden

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
BIG_GOLDEN_ROWS = (30501, 31575, 5459)  # 82, 80 and 79 distinct afterstates


def _encode(f, t):
    return f * 24 + (0 if t == 24 else t)


def _decode(code):
    f, t = divmod(code, 24)
    return (f, 24 if (t == 0 and f <= 5) else t)  # narde_env.py:45-62


def _expressible(m):
    return _decode(_encode(*m)) == m


def reference_afterstates(board, off, ft, player, dice):
    """The ordered afterstate rows of every state, restated over the C oracle.
    Returns a dict: offsets (n + 1,), plays (n,) -- every play of the step,
    inexpressible and duplicate ones included --, inexpressible (n,),
    count1 (n,) list #1's length, and per row codes, board, off, player,
    obs, reward, feat, row_env."""
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft, player, dice = c(board, np.int8), c(off, np.uint8), c(ft, np.uint8), c(player, np.int8), c(dice, np.uint8)
    n = board.shape[0]
    ok = ((dice >= 1) & (dice <= 6)).all(1)
    roll = np.zeros((n, 4), np.uint8)
    roll[:, :2] = np.where(ok[:, None], dice, 1)
    mv, cnt = O.legal_moves(board, ft, player, roll, np.full(n, 2, np.uint8))
    cnt = np.where(ok, cnt, 0)
    # list #1 in list order with duplicates skipped; the entries that get a second list
    firsts, ent_state, ent_move = [], [], []
    for i in range(n):
        first = []
        for r in mv[i, :cnt[i]]:
            m = (int(r[0]), int(r[1]))
            if m not in first:
                first.append(m)
        firsts.append(first)
        if cnt[i] >= 2:
            for m in first:
                ent_state.append(i)
                ent_move.append(m)
    es = np.array(ent_state, np.int64)
    em = np.array(ent_move, np.int8).reshape(-1, 2)
    seconds = []
    if len(es):
        b2, _, ft2 = O.apply_move(board[es], off[es], ft[es], player[es], em)
        rem = np.zeros((len(es), 4), np.uint8)
        for j, (i, (f, t)) in enumerate(zip(ent_state, ent_move)):
            dist = f + 1 if t == 24 else abs(f - t)
            rest = [int(dice[i, 0]), int(dice[i, 1])]
            if dist in rest:
                rest.remove(dist)  # narde_env.py:63-83
            else:
                rest.pop(0)
            rem[j, 0] = rest[0]
        mv2, c2 = O.legal_moves(b2, ft2, player[es], rem, np.ones(len(es), np.uint8))
        seconds = [[(int(r[0]), int(r[1])) for r in mv2[j, :c2[j]]] for j in range(len(es))]
    # the plays, in order
    plays = np.zeros(n, np.int32)
    inexpr = np.zeros(n, np.int32)
    cand_state, cand_codes = [], []
    j = 0
    for i in range(n):
        if cnt[i] == 0:
            continue
        if cnt[i] == 1:  # narde_env.py:41-43: played alone whatever the action
            plays[i] = 1
            cand_state.append(i)
            cand_codes.append((_encode(*firsts[i][0]), 0))
            continue
        for m1 in firsts[i]:
            sec = seconds[j]
            j += 1
            for m2 in (sec if sec else [None]):
                plays[i] += 1
                if _expressible(m1) and (m2 is None or _expressible(m2)):
                    cand_state.append(i)
                    cand_codes.append((_encode(*m1), 0 if m2 is None else _encode(*m2)))
                else:
                    inexpr[i] += 1
    cs = np.array(cand_state, np.int64)
    cc = np.array(cand_codes, np.int16).reshape(-1, 2)
    st = O.step(board[cs], off[cs], ft[cs], player[cs], dice[cs], cc, with_lists=False)
    keep = np.zeros(len(cs), bool)
    counts = np.zeros(n, np.int64)
    seen, cur = set(), -1
    for r in range(len(cs)):
        if cs[r] != cur:
            cur, seen = cs[r], set()
        key = st["board"][r].tobytes() + st["off"][r].tobytes()
        if key not in seen:
            seen.add(key)
            keep[r] = True
            counts[cur] += 1
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    out = dict(offsets=offsets, plays=plays, inexpressible=inexpr, count1=np.asarray(cnt, np.int32),
               row_env=cs[keep].astype(np.int32), codes=cc[keep])
    for k in ("board", "off", "player", "obs", "reward", "terminated"):
        out[k] = st[k][keep]
    out["feat"] = O.tesauro198(out["board"], out["off"], out["player"])
    return out


def golden_states(stride=11, extra=BIG_GOLDEN_ROWS):
    s = golden("steps.npz")
    idx = np.concatenate([np.arange(0, s["board"].shape[0], stride), np.array(extra, np.int64)])
    return s["board"][idx], s["off"][idx], s["first_turn"][idx], s["player"][idx], s["dice"][idx]


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_afterstates.so")
    if not os.path.exists(path):
        import __graft_entry__ as g

        g.build()
    lib = ctypes.CDLL(path)
    lib.hc_afterstates.restype = ctypes.c_int64
    lib.hc_afterstate_key_pairs.restype = ctypes.c_int64
    return lib


def host_afterstates(hc, board, off, ft, player, dice, cap=None):
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft, player, dice = c(board, np.int8), c(off, np.uint8), c(ft, np.uint8), c(player, np.int8), c(dice, np.uint8)
    n = board.shape[0]
    offsets = np.zeros(n + 1, np.int32)
    plays = np.zeros(n, np.int32)

    def run(cap):
        rows = dict(codes=np.zeros((cap, 2), np.int16), board=np.zeros((cap, 24), np.int8),
                    off=np.zeros((cap, 2), np.uint8), player=np.zeros(cap, np.int8), reward=np.zeros(cap, np.int8),
                    feat=np.zeros((cap, 198), np.float32))
        total = hc.hc_afterstates(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice), ctypes.c_int64(cap),
                                  P(offsets), P(plays), P(rows["codes"]), P(rows["board"]), P(rows["off"]),
                                  P(rows["player"]), P(rows["reward"]), P(rows["feat"]))
        return total, rows

    if cap is None:
        cap, _ = run(0)
    total, rows = run(int(cap))
    return dict(rows, offsets=offsets.copy(), plays=plays.copy(), total=total)


def _compare(got, want):
    assert np.array_equal(got["offsets"], want["offsets"])
    assert np.array_equal(got["plays"], want["plays"])
    for k in ("codes", "board", "off", "player", "reward"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["feat"].view(np.uint32), want["feat"].view(np.uint32))


@pytest.fixture(scope="module")
def golden_case():
    st = golden_states()
    return st, reference_afterstates(*st)


@pytest.fixture(scope="module")
def fuzz_case():
    from fuzz_positions import random_positions

    board, off, ft, player, rng = random_positions(3000, 11)
    dice = rng.integers(1, 7, (3000, 2)).astype(np.uint8)
    st = (board, off, ft, player, dice)
    return st, reference_afterstates(*st)


def test_golden_states_equal_the_restatement(hc, golden_case):
    st, want = golden_case
    assert st[0].shape[0] == 4004
    _compare(host_afterstates(hc, *st), want)


def test_random_positions_equal_the_restatement(hc, fuzz_case):
    st, want = fuzz_case
    _compare(host_afterstates(hc, *st), want)


def test_inputs_hold_the_cases_that_matter(golden_case, fuzz_case):
    """Without these the comparisons above could pass vacuously."""
    g, f = golden_case[1], fuzz_case[1]
    rows = lambda w: np.diff(w["offsets"])  # noqa: E731
    assert f["plays"].max() > 256
    assert rows(g).max() > 64 and rows(f).max() > 64
    assert rows(g)[-3:].tolist() == [82, 80, 79]
    for w in (g, f):
        assert ((rows(w) == 0) & (w["count1"] > 0)).any()  # legal moves, none expressible
        assert (w["count1"] == 1).any()
        assert (w["inexpressible"] > 0).any()
        assert (rows(w) < w["plays"] - w["inexpressible"]).any()  # equal afterstates dropped
    assert (g["reward"] == 2).any() or (f["reward"] == 2).any()
    assert (g["reward"] == 1).any() or (f["reward"] == 1).any()
    # the issue's figures for golden[::11] (4,001 states)
    n = 4001
    assert int(g["plays"][:n].sum()) == 78112 and int(g["inexpressible"][:n].sum()) == 9672
    assert int((rows(g)[:n] == 0).sum()) == 144
    assert int(((rows(g)[:n] == 0) & (g["count1"][:n] > 0)).sum()) == 45
    assert int((g["count1"][:n] == 1).sum()) == 150  # list #1 of one entry: played whatever the action

def test_terminal_afterstate_keeps_the_mover(golden_case, fuzz_case):
    for _, w in (golden_case, fuzz_case):
        term = w["reward"] != 0
        if term.any():
            # the winner has 15 off and is still the player of the record
            offs, pl = w["off"][term], w["player"][term]
            assert (np.where(pl == 1, offs[:, 0], offs[:, 1]) == 15).all()


def test_cap_clamps_rows_not_offsets(hc, golden_case):
    st, want = golden_case
    total = int(want["offsets"][-1])
    cap = total // 2
    got = host_afterstates(hc, *st, cap=cap)
    assert got["total"] == total and np.array_equal(got["offsets"], want["offsets"])
    assert np.array_equal(got["codes"], want["codes"][:cap])
    assert np.array_equal(got["feat"], want["feat"][:cap])


def test_bad_dice_give_no_rows(hc, golden_case):
    st = [a[:4].copy() for a in golden_case[0]]
    st[4] = np.array([[0, 3], [7, 1], [2, 0], [9, 9]], np.uint8)
    got = host_afterstates(hc, *st)
    assert got["total"] == 0 and not got["offsets"].any() and not got["plays"].any()
    assert not reference_afterstates(*st)["offsets"].any()


def test_key_is_board_and_off_identity(hc, golden_case, fuzz_case):
    """play_key on every pair of a state's plays (inexpressible ones included)
    against the afterstate records themselves."""
    for st, w in (golden_case, fuzz_case):
        order = np.argsort(-w["plays"])[:150]
        for i in order:
            b, o, f, d = (np.ascontiguousarray(st[k][i]) for k in (0, 1, 2, 4))
            assert hc.hc_afterstate_key_pairs(P(b), P(o), P(f), ctypes.c_int8(int(st[3][i])), P(d)) == 0, int(i)
