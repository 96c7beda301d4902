"""Playout-greedy play (narde_afterstates_records, narde_turn_afterstates_records,
narde_rows_topk, narde_playout_pick, narde_turn_playout_pick; DESIGN.md section
23) on the CPU, through a test-only host build that runs the kernels' shared
functions serially (tests/hostcheck/hostcheck_playout_pick.cpp).

Oracles: the rows and what each leaves are the C oracle's (reference_afterstates
/ enumerate_turns, O.step with the row's codes); the values are the existing
host scored fill's bits (libhostcheck_value.so); the top-K is a numpy stable
sort; the pick is a float64 numpy restatement with the leaves summed in an
explicit sequential loop -- integers, one double division, one rounding, so
equality is exact; the composition is the existing hc_value_playout run one
root at a time.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT

torch = pytest.importorskip("torch")

from test_afterstates_cpu import golden_states, reference_afterstates  # noqa: E402
from test_value_cpu import host_values, make_net  # noqa: E402
from test_value_rollout_cpu import BLACK, NETS, P, endgames, net_in  # noqa: E402
from turn_afterstates_ref import BIG_ROWS, big_state, enumerate_turns  # noqa: E402

FULL = {"ref2": 0, "full4": 1}
T0 = 11  # the envs' ply counter
K = 3    # the k the inputs' cases are stated for
NONE6 = 0xFF


def _load(name):
    path = os.path.join(ROOT, "tests", "hostcheck", "build", name)
    if not os.path.exists(path):
        pytest.fail(f"tests/hostcheck/build/{name} is missing: run __graft_entry__.build()")
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def hc():
    lib = _load("libhostcheck_playout_pick.so")
    lib.hc_records.restype = ctypes.c_int64
    lib.hc_record_none_word6.restype = ctypes.c_uint32
    assert lib.hc_record_none_word6() == NONE6  # narde_rules.h's constant is narde.h's
    return lib


@pytest.fixture(scope="module")
def hc_value():
    return _load("libhostcheck_value.so")


def make_inputs(rules):
    """start_states()' positions -- golden states, fuzz positions, the four
    endgames -- with a roll each, FULL4 with big_state() on 1-1 behind them."""
    from fuzz_positions import random_positions

    g = [np.asarray(a)[::13] for a in golden_states()]
    fb, fo, ff, fp, rng = random_positions(60, 17)
    f = (fb, fo, ff, fp, rng.integers(1, 7, (60, 2)).astype(np.uint8))
    e = endgames() + (np.array([[3, 2], [6, 6], [1, 4], [5, 5]], np.uint8),)
    parts = [g, f, e]
    if rules == "full4":
        b = big_state()
        parts.append((b["board"][None], b["off"][None], b["ft"][None], np.array([b["player"]], np.int8), b["dice"][None]))
    board, off, ft, player, dice = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(5))
    n = board.shape[0]
    return dict(board=board.astype(np.int8), off=off.astype(np.uint8), ft=ft.astype(np.uint8),
                player=player.astype(np.int8), dice=dice.astype(np.uint8), elapsed=(np.arange(n) % 5).astype(np.uint16),
                n=n)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for rules in FULL:
        st = make_inputs(rules)
        args = (st["board"], st["off"], st["ft"], st["player"], st["dice"])
        ref = reference_afterstates(*args) if rules == "ref2" else enumerate_turns(*args)
        out[rules] = (st, ref)
    return out


def host_records(hc, rules, st, net, cap, room=None):
    n = st["n"]
    room = cap + 8 if room is None else room
    keep = []
    col = np.full((room, 2), -77, np.int16) if rules == "ref2" else np.full((room, 4, 2), -77, np.int8)
    o = dict(offsets=np.zeros(n + 1, np.int32), row_env=np.full(room, -77, np.int32), action=col,
             reward=np.full(room, -77, np.int8), value=np.full(room, 12345.0, np.float32),
             records=np.full((room, 8), 0xDEADBEEF, np.uint32))
    nin = net_in(net, keep) if net is not None else None
    o["total"] = hc.hc_records(FULL[rules], ctypes.c_int64(n), P(st["board"]), P(st["off"]), P(st["ft"]), P(st["player"]),
                               P(st["elapsed"]), ctypes.c_uint32(T0), P(st["dice"]), ctypes.c_int64(cap),
                               ctypes.byref(nin) if nin is not None else None, P(o["offsets"]), P(o["row_env"]),
                               P(o["action"]), P(o["reward"]), P(o["value"]), P(o["records"]))
    return o


def decode(hc, records):
    n = records.shape[0]
    d = dict(board=np.zeros((n, 24), np.int8), off=np.zeros((n, 2), np.uint8), ft=np.zeros((n, 2), np.uint8),
             player=np.zeros(n, np.int8), elapsed=np.zeros(n, np.uint16), t=np.zeros(n, np.uint32))
    hc.hc_decode_records(ctypes.c_int64(n), P(np.ascontiguousarray(records)),
                         *(P(d[k]) for k in ("board", "off", "ft", "player", "elapsed", "t")))
    return d


def test_inputs_hold_the_cases_that_matter(cases):
    """From the oracle's rows alone: an env with no row, one with fewer than K
    rows, one with more, and a terminal row that any top-K keeps (its env has
    at most K rows); FULL4's slab tier."""
    for rules, (st, ref) in cases.items():
        rows = np.diff(ref["offsets"])
        assert (rows == 0).any(), rules
        assert ((rows >= 1) & (rows < K)).any(), rules
        assert (rows > K).any(), rules
        term_env = ref["row_env"][ref["reward"] != 0]
        assert len(term_env) and (rows[term_env] <= K).any(), rules
        assert (st["player"][rows > K] == 1).any() and (st["player"][rows > K] == -1).any(), rules
    assert np.diff(cases["full4"][1]["offsets"])[-1] == BIG_ROWS


@pytest.mark.parametrize("rules", list(FULL))
@pytest.mark.parametrize("spec", [NETS[1], NETS[3], None], ids=["H1", "H128", "no-net"])
def test_records_are_what_the_step_leaves(hc, hc_value, cases, rules, spec):
    st, ref = cases[rules]
    total = int(ref["offsets"][-1])
    net = make_net(*spec) if spec is not None else None
    got = host_records(hc, rules, st, net, total)
    assert got["total"] == total and np.array_equal(got["offsets"], ref["offsets"])
    env = ref["row_env"]
    assert np.array_equal(got["row_env"][:total], env)
    column = ref["codes"] if rules == "ref2" else ref["play"]
    assert np.array_equal(got["action"][:total], column)
    assert np.array_equal(got["reward"][:total], ref["reward"])
    d = decode(hc, got["records"][:total])
    for k in ("board", "off", "player"):
        assert np.array_equal(d[k], ref[k]), k
    assert np.array_equal(d["elapsed"], st["elapsed"][env] + 1)
    assert (d["t"] == T0 + 1).all()
    mover_white = st["player"][env] == 1
    if rules == "ref2":  # the C oracle's step with the row's codes
        stp = O.step(st["board"][env], st["off"][env], st["ft"][env], st["player"][env], st["dice"][env], column,
                     with_lists=False)
        assert np.array_equal(d["board"], stp["board"]) and np.array_equal(d["off"], stp["off"])
        assert np.array_equal(d["ft"], stp["first_turn"])
        assert np.array_equal(stp["reward"], ref["reward"])
        assert np.array_equal(d["player"], np.where(stp["terminated"] != 0, st["player"][env], -st["player"][env]))
    # a row moves at least one checker: the mover's first-turn flag is cleared, the other side's kept
    want_ft = st["ft"][env].copy()
    want_ft[mover_white, 0] = 0
    want_ft[~mover_white, 1] = 0
    assert np.array_equal(d["ft"], want_ft)
    # the winner of a terminal row has 15 off and is still the record's mover
    term = ref["reward"] != 0
    assert (np.where(d["player"][term] == 1, d["off"][term, 0], d["off"][term, 1]) == 15).all()
    if net is None:
        assert (got["value"] == np.float32(12345.0)).all()
    else:  # the existing host scored fill's bits
        rows = (st["board"][env], st["off"][env], st["player"][env], ref["board"], ref["off"], ref["player"],
                ref["reward"])
        want = host_values(hc_value, tuple(np.ascontiguousarray(a) for a in rows), net, "white")
        assert np.array_equal(got["value"][:total].view(np.uint32), want.view(np.uint32))
    # nothing at or past cap
    for k in ("row_env", "action", "reward"):
        assert (got[k][total:] == -77).all(), k
    assert (got["records"][total:] == 0xDEADBEEF).all() and (got["value"][total:] == np.float32(12345.0)).all()
    cap = total // 2
    cut = host_records(hc, rules, st, net, cap, room=total)
    assert cut["total"] == total and np.array_equal(cut["offsets"], ref["offsets"])
    assert np.array_equal(cut["records"][:cap], got["records"][:cap])
    assert (cut["records"][cap:] == 0xDEADBEEF).all() and (cut["row_env"][cap:] == -77).all()
    assert (cut["action"][cap:] == -77).all() and (cut["reward"][cap:] == -77).all()


def numpy_topk(offsets, cap, value, black, perspective, k):
    n = len(offsets) - 1
    sel = np.full((n, k), -1, np.int32)
    for e in range(n):
        r0, r1 = int(offsets[e]), min(int(offsets[e + 1]), cap)
        if r1 <= r0:
            continue
        v = value[r0:r1].astype(np.float64)
        x = -v if (perspective == 1 and black[e]) else v
        key = np.where(np.isnan(x), -np.inf, -x)  # NaNs first, then the largest x; stable: the lowest row on ties
        order = np.argsort(key, kind="stable")[:k]
        sel[e, :len(order)] = r0 + order
    return sel


def host_topk(hc, offsets, cap, value, black, perspective, k, records=None):
    n = len(offsets) - 1
    sel = np.full((n, k), -5, np.int32)
    roots = np.full((n * k, 8), 0xABABABAB, np.uint32) if records is not None else None
    hc.hc_rows_topk(ctypes.c_int64(n), P(offsets), ctypes.c_int64(cap), P(value), ctypes.c_int64(1), P(black),
                    perspective, k, P(records), P(sel), P(roots))
    return sel, roots


def host_pick(hc, offsets, cap, value, black, perspective):
    n = len(offsets) - 1
    row = np.full(n, -5, np.int32)
    hc.hc_pick_rows(ctypes.c_int64(n), P(offsets), ctypes.c_int64(cap), P(value), ctypes.c_int64(1), P(black),
                    perspective, P(row))
    return row


@pytest.fixture(scope="module")
def scored(hc, cases):
    out = {}
    for rules, (st, ref) in cases.items():
        total = int(ref["offsets"][-1])
        out[rules] = host_records(hc, rules, st, make_net(*NETS[0]), total, room=total)
    return out


@pytest.mark.parametrize("rules", list(FULL))
@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("perspective", [0, 1])
def test_topk_is_the_stable_sort(hc, cases, scored, rules, k, perspective):
    st, ref = cases[rules]
    got = scored[rules]
    offsets, total = ref["offsets"], int(ref["offsets"][-1])
    black = (st["player"] == -1).astype(np.uint8)
    rows = np.diff(offsets)
    wide = int(np.argmax(rows))
    nan_rows = [int(offsets[wide]) + 1, int(offsets[wide]) + 3]  # two NaNs inside one env: first, in row order
    variants = {"net": got["value"][:total].copy(), "all-ties": np.zeros(total, np.float32)}
    v = got["value"][:total].copy()
    v[nan_rows] = np.nan
    variants["nans"] = v
    cut = int(offsets[wide]) + 2  # a cap inside env `wide`
    for name, value in variants.items():
        for cap in (total, cut):
            sel, roots = host_topk(hc, offsets, cap, value, black, perspective, k, got["records"])
            want = numpy_topk(offsets, cap, value, black, perspective, k)
            assert np.array_equal(sel, want), (name, cap)
            assert np.array_equal(sel[:, 0], host_pick(hc, offsets, cap, value, black, perspective)), (name, cap)
            flat = sel.reshape(-1)
            none = np.zeros(8, np.uint32)
            none[6] = NONE6
            assert np.array_equal(roots[flat >= 0], got["records"][flat[flat >= 0]])
            assert (roots[flat < 0] == none).all()
            alone, nothing = host_topk(hc, offsets, cap, value, black, perspective, k)
            assert nothing is None and np.array_equal(alone, sel)
            if name == "nans" and cap == total and k >= 3:
                assert sel[wide, :2].tolist() == nan_rows
            if name == "all-ties" and cap == total:
                m = np.minimum(rows, k)
                for e in np.flatnonzero(m > 0)[:10]:
                    assert sel[e, :m[e]].tolist() == list(range(offsets[e], offsets[e] + m[e]))


def numpy_pick(sel, value, reward, sums, leaf, trials, black):
    """The float64 restatement: the leaves added one by one in trial order."""
    n, k = sel.shape
    score = np.full((n, k), np.nan, np.float32)
    row = np.full(n, -1, np.int32)
    for e in range(n):
        best, bi = None, -1
        for s in range(k):
            r = int(sel[e, s])
            if r < 0:
                continue
            fin, pts = int(sums[e * k + s, 0]), int(sums[e * k + s, 1])
            if reward[r] != 0:
                sc = value[r]
            elif leaf is None:
                sc = np.float32(np.float64(pts) / np.float64(fin)) if fin > 0 else value[r]
            else:
                S = np.float64(0.0)
                for j in range(trials):
                    if not np.isnan(leaf[e * k + s, j]):
                        S = S + np.float64(leaf[e * k + s, j])
                sc = np.float32((np.float64(pts) + S) / np.float64(trials))
            score[e, s] = sc
            x = -sc if black[e] else sc
            if bi < 0 or (np.isnan(x) and not np.isnan(best)) or (not np.isnan(best) and x > best):
                best, bi = x, s
        row[e] = sel[e, bi] if bi >= 0 else -1
    return row, score


def host_playout_pick(hc, rules, sel, cap, value, reward, column, trials, sums, leaf, black):
    n, k = sel.shape
    word = 4 if rules == "ref2" else 8
    out = np.full((n,) + column.shape[1:], 55, column.dtype)
    row = np.full(n, -5, np.int32)
    score = np.zeros((n, k), np.float32)
    hc.hc_playout_pick(ctypes.c_int64(n), k, P(sel), ctypes.c_int64(cap), P(value), ctypes.c_int64(1), P(reward),
                       P(column), word, trials, P(sums), P(leaf), P(black), P(out), P(row), P(score))
    return out, row, score


@pytest.mark.parametrize("rules", list(FULL))
@pytest.mark.parametrize("with_leaf", [False, True], ids=["finished-mean", "truncated-mean"])
def test_pick_is_the_float64_restatement(hc, cases, scored, rules, with_leaf):
    st, ref = cases[rules]
    got = scored[rules]
    total, trials, k = int(ref["offsets"][-1]), 7, 4
    black = (st["player"] == -1).astype(np.uint8)
    value, reward = got["value"][:total], got["reward"][:total]
    column = np.ascontiguousarray(got["action"][:total])
    sel, _ = host_topk(hc, ref["offsets"], total, value, black, 1, k)
    n = st["n"]
    rng = np.random.default_rng(3)
    fin = rng.integers(0, trials + 1, n * k).astype(np.int32)
    fin[::5] = 0  # no trial finished: the one-ply value
    pts = np.where(fin > 0, rng.integers(-2, 3, n * k), 0).astype(np.int32)  # small: slots tie
    sums = np.ascontiguousarray(np.stack([fin, pts, np.abs(pts), fin * 3], 1).astype(np.int32))
    leaf = None
    if with_leaf:
        leaf = rng.random((n * k, trials)).astype(np.float32) * 2 - 1
        leaf[rng.random((n * k, trials)) < 0.4] = np.nan
        leaf[::7] = np.nan  # every trial finished
        leaf[3::11] = 0.25  # equal leaves: slots tie
    out, row, score = host_playout_pick(hc, rules, sel, total, value, reward, column, trials, sums, leaf, black)
    want_row, want_score = numpy_pick(sel, value, reward, sums, leaf, trials, black)
    assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32))
    assert np.array_equal(row, want_row)
    has = row >= 0
    assert np.array_equal(out[has], column[row[has]])
    assert (out[~has] == (0 if rules == "ref2" else -1)).all() and (~has).any()
    # the cases: finished == 0 falls back to the value, a terminal slot, ties between slots, no candidate
    flat = sel.reshape(-1)
    live = (flat >= 0) & (reward[np.maximum(flat, 0)] == 0)
    if not with_leaf:
        fb = live & (fin == 0)
        assert fb.any() and np.array_equal(score.reshape(-1)[fb].view(np.uint32), value[flat[fb]].view(np.uint32))
    term = (flat >= 0) & (reward[np.maximum(flat, 0)] != 0)
    assert term.any() and np.array_equal(score.reshape(-1)[term], value[flat[term]])
    s2 = np.where(np.isnan(score), np.inf, score)
    assert (np.sort(s2, 1)[:, 0] == np.sort(s2, 1)[:, 1]).any()
    assert np.isnan(score[~has]).all()


@pytest.mark.parametrize("rules", list(FULL))
def test_the_picked_row_is_the_argbest_of_single_root_playouts(hc, cases, scored, rules):
    """The chain on the host -- records, top-K roots, one playout call over all
    roots with common dice, the pick -- against each candidate played out on
    its own through hc_value_playout (n = 1, common dice: the same ids)."""
    from test_value_playout_cpu import host_playout

    st, ref = cases[rules]
    got = scored[rules]
    total, trials, k, plies, id_base = int(ref["offsets"][-1]), 4, 3, 40, 23
    white, blk = make_net(*NETS[0]), make_net(*BLACK[80])
    rows = np.diff(ref["offsets"])
    n = st["n"] - (1 if rules == "full4" else 0)  # (big_state()'s playouts are test_value_playout_cpu's)
    envs = np.concatenate([np.flatnonzero((rows[:n] > k))[:3], np.flatnonzero(rows[:n] == 0)[:1],
                           np.flatnonzero((rows[:n] >= 1) & (rows[:n] < k))[:2], np.arange(n - 4, n)])
    black = (st["player"] == -1).astype(np.uint8)
    value, reward = got["value"][:total], got["reward"][:total]
    sel, roots = host_topk(hc, ref["offsets"], total, value, black, 1, k, got["records"])
    sel, roots = np.ascontiguousarray(sel[envs]), np.ascontiguousarray(roots.reshape(-1, k, 8)[envs].reshape(-1, 8))
    d = decode(hc, roots)
    state = (d["board"], d["off"], d["ft"], d["player"])
    res = host_playout(hc, rules, state, T0 + 1, trials, plies, white, blk, id_base=id_base, common=True)
    column = np.ascontiguousarray(got["action"][:total])
    _, row, score = host_playout_pick(hc, rules, sel, total, value, reward, column, trials, res["sums"], None,
                                      np.ascontiguousarray(black[envs]))
    picked_some = 0
    for i, e in enumerate(envs):
        best, want = None, -1
        for s in range(k):
            r = int(sel[i, s])
            if r < 0:
                continue
            if reward[r] != 0:
                sc = float(value[r])
            else:
                one = host_playout(hc, rules, tuple(a[i * k + s:i * k + s + 1] for a in state), T0 + 1, trials, plies,
                                   white, blk, id_base=id_base, common=True)
                assert np.array_equal(one["sums"][0], res["sums"][i * k + s])
                f, p = int(one["sums"][0, 0]), int(one["sums"][0, 1])
                sc = float(np.float32(p / f)) if f > 0 else float(value[r])
            x = -sc if black[e] else sc
            if best is None or x > best:
                best, want = x, r
        assert row[i] == want, (rules, int(e))
        picked_some += want >= 0
    assert picked_some >= 6
