"""FULL4 whole-turn afterstates (narde_rules.h "FULL4 turn afterstates": the
per-node functions of k_turn_count / k_turn_fill) on the CPU, through a
test-only host build that walks each env's levels serially
(tests/hostcheck/hostcheck_turn_afterstates.cpp), against the enumerator over
oracle.full4_turn (tests/turn_afterstates_ref.py).  Every comparison is bit
for bit, floats included.
"""
import ctypes
import os

import numpy as np
import pytest

import turn_afterstates_ref as R
from conftest import ROOT, golden

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_turn_afterstates.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_turn_afterstates.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    lib.hc_turn_afterstates.restype = ctypes.c_int64
    lib.hc_turn_key_pairs.restype = ctypes.c_int64
    return lib


def host_rows(lib, s, cap=None):
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft = c(s["board"], np.int8), c(s["off"], np.uint8), c(s["ft"], np.uint8)
    player, dice = c(s["player"], np.int8), c(s["dice"], np.uint8)
    n = board.shape[0]
    offsets = np.zeros(n + 1, np.int32)
    front = np.zeros(n, np.int32)
    z = np.zeros(1, np.int8)
    if cap is None:
        cap = int(lib.hc_turn_afterstates(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice),
                                          ctypes.c_int64(0), P(offsets), P(front), P(z), P(z), P(z), P(z), P(z), P(z)))
    out = dict(offsets=offsets, front=front, play=np.full((cap, 4, 2), 99, np.int8), board=np.zeros((cap, 24), np.int8),
               off=np.zeros((cap, 2), np.uint8), player=np.zeros(cap, np.int8), reward=np.zeros(cap, np.int8),
               feat=np.zeros((cap, 198), np.float32))
    total = lib.hc_turn_afterstates(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice), ctypes.c_int64(cap),
                                    P(offsets), P(front), P(out["play"]), P(out["board"]), P(out["off"]),
                                    P(out["player"]), P(out["reward"]), P(out["feat"]))
    assert total == offsets[n]
    return out


def check(lib, s):
    ref = R.enumerate_turns(s["board"], s["off"], s["ft"], s["player"], s["dice"])
    got = host_rows(lib, s)
    assert np.array_equal(got["offsets"], ref["offsets"])
    for k in ("play", "board", "off", "player", "reward"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["feat"].tobytes() == ref["feat"].tobytes()
    return ref, got


@pytest.fixture(scope="module")
def selfplay(hc):
    s = R.selfplay_states()
    return s, check(hc, s)


def test_selfplay_states(selfplay):
    s, (ref, got) = selfplay
    n = len(s["player"])
    cnt = np.diff(ref["offsets"])
    # the sample: 1,920 states, 10.2 rows on average, 131 at most, 15 with no row
    assert n == 1920 and int(cnt.sum()) == 19592 and cnt.max() == 131 and (cnt == 0).sum() == 15
    assert (ref["plays"] > cnt).any()  # plays that leave the same position
    assert set(np.unique(ref["max_dice"])) >= {0, 1, 2, 3, 4}


@pytest.fixture(scope="module")
def fuzz(hc):
    from fuzz_positions import turn_states

    s = turn_states(1000, 505)
    return s, check(hc, s)


def test_positions_off_selfplay(fuzz):
    """Run-heavy boards, half of them on a double, and bear-off endgames
    (tests/fuzz_positions.py): what random play does not reach."""
    s, (ref, got) = fuzz
    cnt = np.diff(ref["offsets"])
    rew = ref["reward"]
    print(f"states {len(cnt)}, rows {int(cnt.sum())}, above 256 rows {int((cnt > 256).sum())}, most rows {int(cnt.max())}, "
          f"most plays {int(ref['plays'].max())}, no row {int((cnt == 0).sum())}, reward 1 / 2 rows "
          f"{int((rew == 1).sum())} / {int((rew == 2).sum())}")
    assert (cnt > 256).sum() >= 100
    # each of those has a level above the device's fast frontier (256 nodes): the overflow list's
    assert (got["front"][cnt > 256] > 256).all()
    assert set(np.unique(ref["max_dice"])) >= {0, 1, 2, 3, 4}
    assert (rew == 1).any() and (rew == 2).any()
    assert (cnt == 0).any()
    assert (ref["plays"] > cnt).any()


def test_golden_full4_states(hc):
    g = golden("full4.npz")
    check(hc, R.golden_states(g))


def test_start_position_all_dice(hc):
    s = R.start_states()
    ref, _ = check(hc, s)
    cnt = dict(zip(map(tuple, s["dice"]), np.diff(ref["offsets"])))
    # one head move a turn: the lone head checker walks both dice (one row);
    # doubles: it walks up to four steps while the landings are free
    assert cnt[(2, 1)] == 1 and cnt[(5, 2)] == 1
    # a first-turn 3-3 / 4-4 / 6-6 takes two checkers off the head
    two = ref["play"][ref["offsets"][:-1][[i for i, d in enumerate(map(tuple, s["dice"])) if d in ((3, 3), (4, 4), (6, 6))]]]
    assert ((two[:, :, 0] == 23).sum(1) == 2).all()


def test_edge_states(hc):
    s = R.edge_states()
    ref, _ = check(hc, s)
    cnt = np.diff(ref["offsets"])
    rew = [ref["reward"][ref["offsets"][i]:ref["offsets"][i + 1]].tolist() for i in range(len(cnt))]
    # bearing the last two off is one row among those that leave a checker on
    assert sorted(rew[0]) == [0, 0, 1] and sorted(rew[1]) == [0, 0, 2] and rew[2] == [2] and rew[3] == [1]
    assert 2 in rew[4] and 1 not in rew[4]
    # the mover is flipped unless the turn ended the game
    for i in (0, 1, 4):
        sl = slice(ref["offsets"][i], ref["offsets"][i + 1])
        assert np.array_equal(ref["player"][sl] == s["player"][i], ref["reward"][sl] != 0)
    pl = lambda i: ref["play"][ref["offsets"][i]].tolist()  # noqa: E731
    assert cnt[5] == 1 and pl(5)[0] == [23, 6] and pl(5)[1] == [-1, -1]
    assert cnt[6] == 1 and pl(6)[0] == [23, 1] and pl(6)[1] == [-1, -1]
    assert cnt[7] == 1 and pl(7)[0] == [23, 6] and ref["max_dice"][7] == 1
    assert cnt[8] == 0 and cnt[9] == 0 and cnt[10] == 0
    assert ref["max_dice"][11] == 2 and cnt[11] == 1


def test_largest_position(hc):
    s = R.big_states()
    ref, got = check(hc, s)
    assert ref["offsets"][1] == R.BIG_ROWS and ref["plays"][0] == R.BIG_PLAYS
    lib_max = hc.hc_turn_aft_max()
    assert R.BIG_ROWS <= got["front"][0] <= lib_max


def test_cap_leaves_tail_untouched(hc):
    s = R.edge_states()
    full = host_rows(hc, s)
    total = int(full["offsets"][-1])
    part = host_rows(hc, s, cap=total - 2)
    assert np.array_equal(part["offsets"], full["offsets"])
    assert np.array_equal(part["play"], full["play"][:total - 2])


def test_dedupe_key_matches_records(hc, selfplay):
    """turn_path_key against the position records on every sub-move sequence
    (all pairs, through the two maps) of the 100 largest sample states, the
    start position's doubles and the 2,065-row position."""
    s, (ref, _) = selfplay
    big = np.argsort(-np.diff(ref["offsets"]), kind="stable")[:100]
    sets = [{k: s[k][big] for k in s}, R.start_states(), R.edge_states(), R.big_states()]
    paths = 0
    for st in sets:
        for i in range(len(st["player"])):
            if not ((st["dice"][i] >= 1) & (st["dice"][i] <= 6)).all():
                continue
            np_ = ctypes.c_int64(0)
            c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
            bad = hc.hc_turn_key_pairs(P(c(st["board"][i], np.int8)), P(c(st["off"][i], np.uint8)), P(c(st["ft"][i], np.uint8)),
                                       ctypes.c_int8(int(st["player"][i])), P(c(st["dice"][i], np.uint8)), ctypes.byref(np_))
            assert bad == 0, (i, st["board"][i], st["dice"][i])
            paths += np_.value
    assert paths > R.BIG_PLAYS
