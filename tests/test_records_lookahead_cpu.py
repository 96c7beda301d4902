"""The two-ply values of given records (narde_records_lookahead,
narde_turn_records_lookahead) and the pick over given slot scores
(narde_slot_pick) on the CPU, through a test-only host
build that runs the kernels' shared functions serially on given records
(tests/hostcheck/hostcheck_records_lookahead.cpp).

Two oracles.  On the public records of a roll's rows the values must be the
existing host lookahead's bit for bit (terminal rows' records: NaN).  On
hand-made positions they are compared with the float64 pipelines of
tests/lookahead_ref.py / tests/turn_lookahead_ref.py over the C oracle, within
those tests' own rule: TOL_FACTOR (8) x E, E = max |pipeline in torch float32
- in float64| on the same positions, floored at one float32 ulp of the largest
magnitude compared -- the reference's own rounding, never the code under
test's.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
from conftest import ROOT

torch = pytest.importorskip("torch")

import lookahead_ref as LR  # noqa: E402
import test_lookahead_cpu as T2  # noqa: E402
import test_turn_lookahead_cpu as T4  # noqa: E402
import turn_afterstates_ref as R  # noqa: E402
import turn_lookahead_ref as TL  # noqa: E402
from test_afterstates_cpu import reference_afterstates  # noqa: E402
from test_value_cpu import TOL_FACTOR, make_net  # noqa: E402

P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
NETS = T2.NETS
NONE_RECORD = np.array([0, 0, 0, 0, 0, 0, 0xFF, 0], np.uint32)


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_records_lookahead.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_records_lookahead.so is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    lib.hc_lookahead.restype = ctypes.c_int64
    lib.hc_turn_lookahead.restype = ctypes.c_int64
    return lib


def pack_records(hc, board, off, ft, player, elapsed=None, t=None):
    """Public records u32 (n, 8) of positions; elapsed u16 (n,), t u32 (n,) or None (0)."""
    c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft, player = c(board, np.int8), c(off, np.uint8), c(ft, np.uint8), c(player, np.int8)
    elapsed, t = c(elapsed, np.uint16), c(t, np.uint32)
    n = board.shape[0]
    rec = np.zeros((n, 8), np.uint32)
    hc.hc_pack_records(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(elapsed), P(t), P(rec))
    return rec


def host_records_lookahead(hc, full, records, net, dice_mode=0):
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    records = c(records, np.uint32)
    n, per = records.shape[0], 21 if full else 36
    w1t = c(net.l1.weight.detach().numpy().T, np.float32)
    b1, w2, b2 = (c(a.detach().numpy().reshape(-1), np.float32) for a in (net.l1.bias, net.l2.weight, net.l2.bias))
    o = dict(value=np.full(n, 7.0, np.float32), replies=np.zeros((n, per), np.int32),
             front=np.zeros((n, per), np.int32), best=np.zeros((n, per), np.float32))
    hc.hc_records_lookahead(int(full), ctypes.c_int64(n), P(records), dice_mode, P(w1t), ctypes.c_int64(w1t.shape[1]),
                            P(b1), P(w2), P(b2), net.hidden, HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act],
                            *(P(o[k]) for k in ("value", "replies", "front", "best")))
    return o


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the rows' records against the full search
@pytest.fixture(scope="module")
def rows2(hc):
    return T2.lookahead_states()


@pytest.fixture(scope="module")
def rows4(hc):
    return T4.lookahead_states()


def _rows_case(hc, full, st, net, dice_mode, seed):
    got = (T4.host_lookahead if full else T2.host_lookahead)(hc, st, net, dice_mode=dice_mode)
    rng = np.random.default_rng(seed)
    n = got["total"]
    rec = pack_records(hc, got["board"], got["off"], got["ft"], got["player"],
                       rng.integers(1, 2 ** 16, n), rng.integers(1, 2 ** 32, n, dtype=np.uint64))
    return got, rec


@pytest.mark.parametrize("full", (False, True), ids=("ref2", "full4"))
@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_rows_records_give_the_full_searchs_bits(hc, rows2, rows4, full, spec):
    net = make_net(*spec)
    for dice_mode in ((0, 1) if spec == NETS[0] else (0,)):  # NODOUBLES once
        got, rec = _rows_case(hc, full, rows4 if full else rows2, net, dice_mode, 5)
        live = got["reward"] == 0
        assert live.any() and (~live).any() and got["total"] > 200
        assert (rec[:, 7] != 0).all() and ((rec[:, 6] >> 16) != 0).all()  # the ply counter and elapsed are set
        out = host_records_lookahead(hc, full, rec, net, dice_mode)
        assert np.array_equal(bits(out["value"][live]), bits(got["value"][live]))
        assert np.isnan(out["value"][~live]).all() and not np.isnan(out["value"][live]).any()
        cols = slice(None)
        assert np.array_equal(bits(out["best"][live][:, cols]), bits(got["best"][live][:, cols]))
        assert np.array_equal(out["replies"][live], got["replies"][live].astype(np.int32))
        assert (out["replies"][~live] == -1).all()


@pytest.mark.parametrize("full", (False, True), ids=("ref2", "full4"))
def test_the_ply_counter_and_elapsed_change_no_bit(hc, rows2, rows4, full):
    net = make_net(*NETS[0])
    got, rec = _rows_case(hc, full, rows4 if full else rows2, net, 0, 6)
    zero = pack_records(hc, got["board"], got["off"], got["ft"], got["player"])
    assert not zero[:, 7].any() and not (zero[:, 6] >> 16).any()
    assert np.array_equal(zero[:, :6], rec[:, :6]) and np.array_equal(zero[:, 6] & 0xFFFF, rec[:, 6] & 0xFFFF)
    a, b = host_records_lookahead(hc, full, zero, net), host_records_lookahead(hc, full, rec, net)
    assert np.array_equal(bits(a["value"]), bits(b["value"])) and np.array_equal(bits(a["best"]), bits(b["best"]))


@pytest.mark.parametrize("full", (False, True), ids=("ref2", "full4"))
def test_finished_records_are_nan(hc, full):
    net = make_net(*NETS[0])
    board = np.zeros((4, 24), np.int8)
    off = np.array([[15, 3], [0, 15], [15, 0], [14, 14]], np.uint8)
    board[0, 13], board[1, 5], board[2, 12], board[3, 0], board[3, 14] = -12, 15, -15, 1, -1
    rec = pack_records(hc, board, off, np.zeros((4, 2), np.uint8), np.array([1, -1, -1, 1], np.int8),
                       t=np.array([0, 9, 0, 0]))
    rec = np.concatenate([rec, NONE_RECORD[None]])
    out = host_records_lookahead(hc, full, rec, net)
    assert np.isnan(out["value"][[0, 1, 2, 4]]).all() and (out["replies"][[0, 1, 2, 4]] == -1).all()
    assert np.isfinite(out["value"][3]) and (out["replies"][3] >= 0).all()  # 14 off on both sides: live


# ------------------------------------------------------------------ hand-made positions against the C oracle
def positions2():
    from fuzz_positions import endgame_boards, random_positions

    board, off, ft, player, _ = random_positions(40, 29)
    eb, eoff = endgame_boards(12, 31)  # white to move, bearing off
    # one roll from the end: the mover has 13 or 14 off, so some replies end the game (worth 1 and 2)
    last = np.zeros((4, 24), np.int8)
    loff = np.array([[14, 0], [13, 2], [0, 14], [5, 13]], np.uint8)
    last[0, 2], last[0, 15] = 1, -15
    last[1, 0], last[1, 3], last[1, 16] = 1, 1, -13
    last[2, 12 + 1], last[2, 4] = -1, 15
    last[3, 12 + 0], last[3, 12 + 5], last[3, 6] = -1, -1, 10
    lplayer = np.array([1, 1, -1, -1], np.int8)
    return tuple(np.ascontiguousarray(np.concatenate(p)) for p in
                 ((board, eb, last), (off, eoff, loff), (ft, np.zeros((16, 2), np.uint8)),
                  (player, np.ones(12, np.int8), lplayer)))


def replies2(rec, dice_mode):
    """test_lookahead_cpu.reference_case's reply loop with the positions given."""
    n, out = len(rec[3]), []
    for a, b in LR.rolls_of(dice_mode):
        d = np.tile(np.array([a, b], np.uint8), (n, 1))
        rep = reference_afterstates(*rec, d)
        ps = O.step(*rec, d, np.zeros((n, 2), np.int16), with_lists=False)
        rep.update(pass_feat=O.tesauro198(ps["board"], ps["off"], ps["player"]), pass_reward=ps["reward"],
                   pass_player=ps["player"])
        out.append(rep)
    return out


@pytest.fixture(scope="module")
def hand2():
    rec = positions2()
    return rec, replies2(rec, "all36")


def _check(out, want, w32, m64, cols, what):
    E = LR.error_bound(w32, want)
    tol = TOL_FACTOR * E
    assert np.ptp(want) > 1e3 * tol  # the values differ: a wrong reply would show
    err = float(np.abs(out["value"].astype(np.float64) - want).max())
    errm = float(np.abs(out["best"][:, cols].astype(np.float64) - m64).max())
    print(f"{what}: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E; per roll {errm:.3e} = {errm / E:.2f} E")
    assert err <= tol, (err, tol)  # (E is the means' rounding: the per-roll figure is printed, as in those tests)


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_hand_made_positions_ref2(hc, hand2, spec):
    rec, replies = hand2
    net = make_net(*spec)
    black = rec[3] == -1
    assert black.any() and (~black).any()
    cnt = np.stack([np.diff(r["offsets"]) for r in replies], 1)
    assert (cnt == 0).any() and any((r["reward"] != 0).any() for r in replies)  # no-reply rolls, terminal replies
    rng = np.random.default_rng(2)
    records = pack_records(hc, *rec, rng.integers(0, 2 ** 16, len(black)), rng.integers(0, 2 ** 32, len(black), dtype=np.uint64))
    out = host_records_lookahead(hc, False, records, net)
    assert np.array_equal(out["replies"], cnt)
    want, w32, m64 = LR.two_ply(net, replies, black)
    _check(out, want, w32, m64, slice(None), f"ref2 {spec[:3]}")
    # NODOUBLES: the 30-roll mean, not the 36-roll one
    keep = [i for i, (a, b) in enumerate(LR.rolls_of("all36")) if a != b]
    out30 = host_records_lookahead(hc, False, records, net, dice_mode=1)
    w30, w32_30, m30 = LR.two_ply(net, [replies[i] for i in keep], black)
    _check(out30, w30, w32_30, m30, keep, f"ref2 nodoubles {spec[:3]}")
    assert (out30["replies"][:, [6 * k + k for k in range(6)]] == -1).all()
    assert np.abs(want - w30).max() > 1e3 * TOL_FACTOR * LR.error_bound(w32_30, w30)


def positions4():
    from fuzz_positions import spread_replier_states, turn_states

    s, t = spread_replier_states(10, 711), turn_states(10, 713)
    return tuple(np.ascontiguousarray(np.concatenate([s[k], t[k]])) for k in ("board", "off", "ft", "player"))


def replies4(rec, dice_mode):
    """turn_lookahead_ref.reference_case's reply loop with the positions given."""
    n, out, ks = len(rec[3]), [], TL.rolls_of(dice_mode)
    for k in ks:
        a, b = TL.ROLLS[k]
        d = np.tile(np.array([a, b], np.uint8), (n, 1))
        rep = R.enumerate_turns(*rec, d)
        ps = TL.oracle_step(*rec, d, np.full((n, 4, 2), -1, np.int8))
        rep.update(pass_feat=O.tesauro198(ps["board"], ps["off"], ps["player"]), pass_reward=ps["reward"],
                   pass_player=ps["player"])
        out.append(rep)
    return out, ks


@pytest.fixture(scope="module")
def hand4():
    rec = positions4()
    replies, ks = replies4(rec, "all36")
    return rec, replies, ks


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_hand_made_positions_full4(hc, hand4, spec):
    rec, replies, ks = hand4
    net = make_net(*spec)
    black = rec[3] == -1
    assert black.any() and (~black).any()
    cnt = np.stack([np.diff(r["offsets"]) for r in replies], 1)
    assert (cnt == 0).any() and cnt.max() > 256  # passes; a final level beyond the fast frontier
    rng = np.random.default_rng(3)
    records = pack_records(hc, *rec, rng.integers(0, 2 ** 16, len(black)), rng.integers(0, 2 ** 32, len(black), dtype=np.uint64))
    out = host_records_lookahead(hc, True, records, net)
    assert np.array_equal(out["replies"][:, ks], cnt)
    want, w32, m64 = TL.two_ply_weighted(net, replies, ks, black)
    _check(out, want, w32, m64, ks, f"full4 {spec[:3]}")
    k15 = TL.rolls_of("nodoubles")
    out15 = host_records_lookahead(hc, True, records, net, dice_mode=1)
    w15, w32_15, m15 = TL.two_ply_weighted(net, [replies[ks.index(k)] for k in k15], k15, black)
    _check(out15, w15, w32_15, m15, k15, f"full4 nodoubles {spec[:3]}")
    assert (out15["replies"][:, [k for k in ks if k not in k15]] == -1).all()
    assert np.abs(want - w15).max() > 1e3 * TOL_FACTOR * LR.error_bound(w32_15, w15)


@pytest.mark.parametrize("points, lo, hi", ((TL.TIER_LDS_POINTS, 257, 2048), (TL.TIER_SLAB_POINTS, 2049, 5220)),
                         ids=("lds-tier", "slab-tier"))
def test_overflow_tier_positions_full4(hc, points, lo, hi):
    """The positions tier_state()'s rows leave: their reply walks outgrow the
    256-node frontier (the LDS tier) or the 2,048-node one (the slab tier)."""
    c = TL.reference_case(TL.tier_state(points))
    rec, ks = c["rec"], c["ks"]
    net = make_net(*NETS[0])
    records = pack_records(hc, *rec, t=np.full(len(rec[3]), 77))
    out = host_records_lookahead(hc, True, records, net)
    top = int(out["front"].max())
    assert lo <= top <= hi, top
    cnt = np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1)
    assert np.array_equal(out["replies"][:, ks], cnt)
    want, w32, m64 = TL.two_ply_weighted(net, c["replies"], ks, rec[3] == -1)
    E = LR.error_bound(w32, want)
    err = float(np.abs(out["value"].astype(np.float64) - want).max())
    errm = float(np.abs(out["best"][:, ks].astype(np.float64) - m64).max())
    print(f"tier {lo}..{hi}: largest level {top}, E = {E:.3e}, max error = {err:.3e}, per roll {errm:.3e}")
    assert err <= TOL_FACTOR * E


# ------------------------------------------------------------------ the slot pick
def slot_case(seed, n=300, k=5, cap=400, word=4):
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, cap, (n, k)).astype(np.int32)
    short = rng.integers(0, k + 1, n)  # candidates an env has: 0 .. k
    short[:3] = (0, 1, k)
    sel[np.arange(k)[None] >= short[:, None]] = -1
    value = rng.choice(np.array([-2, -1, 1, 2], np.float32), cap)
    reward = np.where(rng.random(cap) < 0.25, rng.integers(1, 3, cap), 0).astype(np.int8)
    score = rng.choice(np.linspace(-1, 1, 7).astype(np.float32), (n, k))  # few levels: ties
    column = rng.integers(1, 2 ** 31, (cap, word // 4), dtype=np.int64).astype(np.uint32)
    black = (rng.random(n) < 0.5).astype(np.uint8)
    return dict(n=n, k=k, cap=cap, word=word, sel=sel, value=value, reward=reward, score=score, column=column, black=black)


def numpy_slot_pick(c, score):
    """The pick restated: NaN for no candidate, a terminal row's value, else the
    slot's score; white the largest, black the smallest; the lowest slot on
    ties; a NaN score beats every number (the lowest slot among NaNs)."""
    n, k = c["n"], c["k"]
    sc = np.full((n, k), np.nan, np.float32)
    slot = np.full(n, -1, np.int64)
    for e in range(n):
        best = None
        for s in range(k):
            r = c["sel"][e, s]
            if r < 0:
                continue
            sc[e, s] = c["value"][r] if c["reward"][r] != 0 else score[e, s]
            x = -sc[e, s] if c["black"][e] else sc[e, s]
            if best is None:
                best, slot[e] = x, s
            elif np.isnan(x) or np.isnan(best):
                if np.isnan(x) and not np.isnan(best):
                    best, slot[e] = x, s
            elif x > best:
                best, slot[e] = x, s
    row = np.where(slot >= 0, c["sel"][np.arange(n), np.maximum(slot, 0)], -1).astype(np.int32)
    none = np.uint32(0xFFFFFFFF if c["word"] == 8 else 0)
    out = np.where((row >= 0)[:, None], c["column"][np.maximum(row, 0)], none)
    return out, row, sc, slot


def host_slot_pick(hc, c, score):
    out = np.zeros((c["n"], c["word"] // 4), np.uint32)
    row, sc = np.zeros(c["n"], np.int32), np.zeros((c["n"], c["k"]), np.float32)
    score = np.ascontiguousarray(score, np.float32)
    hc.hc_slot_pick(ctypes.c_int64(c["n"]), c["k"], P(c["sel"]), ctypes.c_int64(c["cap"]), P(c["value"]),
                    ctypes.c_int64(1), P(c["reward"]), P(c["column"]), c["word"], P(score), P(c["black"]), P(out), P(row),
                    P(sc))
    return out, row, sc


@pytest.mark.parametrize("word", (4, 8), ids=("ref2", "full4"))
@pytest.mark.parametrize("k", (1, 3, 8))
def test_slot_pick_is_the_numpy_restatement(hc, word, k):
    c = slot_case(40 + k, k=k, word=word)
    score = c["score"].copy()
    score[np.random.default_rng(k).random(score.shape) < 0.1] = np.nan  # NaN scores
    out, row, sc = host_slot_pick(hc, c, score)
    wout, wrow, wsc, slot = numpy_slot_pick(c, score)
    assert np.array_equal(row, wrow) and np.array_equal(out, wout)
    assert np.array_equal(np.isnan(sc), np.isnan(wsc)) and np.array_equal(bits(sc)[~np.isnan(sc)], bits(wsc)[~np.isnan(wsc)])
    assert (row == -1).any() and (out[row == -1] == (0xFFFFFFFF if word == 8 else 0)).all()  # an env with no candidate
    live = c["sel"] >= 0
    term = live & (c["reward"][np.maximum(c["sel"], 0)] != 0)
    assert term.any() and np.array_equal(sc[term], c["value"][c["sel"][term]])  # terminal slots take value[r]
    picked_nan = np.isnan(sc[np.arange(c["n"]), np.maximum(slot, 0)]) & (slot >= 0)
    assert picked_nan.any()  # a NaN score is taken, as the picks take it
    if k > 1:
        best = np.where(c["black"][:, None] != 0, -sc, sc)
        ties = (np.nan_to_num(best, nan=-9) == np.nanmax(np.nan_to_num(best, nan=-9), 1)[:, None]).sum(1) > 1
        assert ties.any()  # ties, which go to the lowest slot


@pytest.mark.parametrize("k", (1, 3, 8))
def test_slot_pick_is_the_playout_pick_of_one_leaf(hc, k):
    """playout_pick_slot with trials = 1, zero sums and leaf = slot_score: its
    truncated mean (0 + leaf) / 1 returns the leaf itself."""
    c = slot_case(60 + k, k=k)
    out, row, sc = host_slot_pick(hc, c, c["score"])
    sums = np.zeros((c["n"] * k, 4), np.int32)
    slot, psc = np.zeros(c["n"], np.int32), np.zeros((c["n"], k), np.float32)
    hc.hc_playout_pick_slots(ctypes.c_int64(c["n"]), k, P(c["sel"]), ctypes.c_int64(c["cap"]), P(c["value"]),
                             ctypes.c_int64(1), P(c["reward"]), 1, P(sums), P(c["score"]), P(c["black"]), P(slot), P(psc))
    prow = np.where(slot >= 0, c["sel"][np.arange(c["n"]), np.maximum(slot, 0)], -1)
    assert np.array_equal(row, prow)
    assert np.array_equal(np.isnan(sc), np.isnan(psc)) and np.array_equal(bits(sc)[~np.isnan(sc)], bits(psc)[~np.isnan(psc)])
