"""The value MLP's shared arithmetic (narde_rules.h "value MLP": what the
scored fill kernels run) on the CPU, through a test-only host build that
takes a wave's lanes in turn (tests/hostcheck/hostcheck_value.cpp).

1. The column lists are exact: a row's (column, new value) list applied to
   its root's tes_value row gives the row's tes_value row bit for bit, no
   listed column is unchanged, and a record's own list is its non-zero
   columns in ascending order.
2. The values: against torch's float64 evaluation of ValueMLP.forward on
   O.tesauro198 rows, within tol = 8 x E, E = max |torch-fp32 - torch-fp64|
   on the same rows -- the reference's own rounding, measured here, never
   the code under test's.  A dropped or misplaced column moves a value by
   about |W| x 0.5 ~ 1e-2, four orders of magnitude above tol.  Terminal
   rows equal the outcome rule exactly.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import turn_afterstates_ref as R
from conftest import ROOT
from test_afterstates_cpu import golden_states, reference_afterstates

torch = pytest.importorskip("torch")

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
# (hidden, g_hid, g_out, seed)
NETS = [(80, "sigmoid", "sigmoid", 1), (128, "tanh", "none", 2), (1, "relu", "none", 3), (65, "relu", "tanh", 4),
        (64, "sigmoid", "sigmoid", 5)]
TOL_FACTOR = 8


def make_net(hidden, hidden_act, out_act, seed, scale=4.0):
    """torch's default init, l1 and l2.weight scaled so that the values of an
    env's rows differ."""
    from gym_narde.value_net import ValueMLP

    torch.manual_seed(seed)
    net = ValueMLP(hidden, hidden_act, out_act)
    with torch.no_grad():
        net.l1.weight.mul_(scale)
        net.l1.bias.mul_(scale)
        net.l2.weight.mul_(scale)
    return net


def torch_values(net, feat):
    """(fp64 values, E = max |fp32 - fp64|) of net.forward on feat (numpy)."""
    import copy

    x = torch.from_numpy(np.ascontiguousarray(feat))
    with torch.no_grad():
        v32 = net(x).double()
        v64 = copy.deepcopy(net).double()(x.double())
    return v64.numpy(), float((v32 - v64).abs().max())


def outcome(reward, player, perspective):
    """A terminal row's value: reward for the side that moved (the row's
    player: not flipped after a terminal step), negated for black in white's
    perspective."""
    r = reward.astype(np.float32)
    return np.where((player == -1) & (perspective == "white"), -r, r)


@pytest.fixture(scope="module")
def hc():
    path = os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_value.so")
    if not os.path.exists(path):
        pytest.fail("tests/hostcheck/build/libhostcheck_value.so is missing: run __graft_entry__.build()")
    return ctypes.CDLL(path)


def rows_of(st, ref):
    """(root board, off, player, row board, off, player, reward) per row."""
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    e = ref["row_env"]
    return (c(np.asarray(st[0])[e], np.int8), c(np.asarray(st[1])[e], np.uint8), c(np.asarray(st[3])[e], np.int8),
            c(ref["board"], np.int8), c(ref["off"], np.uint8), c(ref["player"], np.int8), c(ref["reward"], np.int8))


@pytest.fixture(scope="module")
def ref2_case():
    st = golden_states()
    ref = reference_afterstates(*st)
    return rows_of(st, ref), ref


@pytest.fixture(scope="module")
def full4_case():
    s = R.concat(R.selfplay_states(), R.big_states())
    ref = R.enumerate_turns(s["board"], s["off"], s["ft"], s["player"], s["dice"])
    return rows_of((s["board"], s["off"], s["ft"], s["player"]), ref), ref


def host_lists(hc, rows):
    n = len(rows[6])
    out = dict(cnt=np.zeros(n, np.int32), col=np.full((n, 16), -1, np.int32), oldv=np.zeros((n, 16), np.float32),
               newv=np.zeros((n, 16), np.float32), feat_root=np.zeros((n, 198), np.float32),
               feat_row=np.zeros((n, 198), np.float32), nz_cnt=np.zeros(n, np.int32),
               nz_col=np.full((n, 48), -1, np.int32), nz_val=np.zeros((n, 48), np.float32))
    out["most"] = hc.hc_value_lists(ctypes.c_int64(n), *(P(a) for a in rows[:6]), *(P(out[k]) for k in (
        "cnt", "col", "oldv", "newv", "feat_root", "feat_row", "nz_cnt", "nz_col", "nz_val")))
    return out


def check_lists(got, rows, ref):
    n = len(rows[6])
    # tes_value's rows are the oracle's
    assert got["feat_row"].tobytes() == np.ascontiguousarray(ref["feat"]).tobytes()
    assert got["feat_root"].tobytes() == O.tesauro198(rows[0], rows[1], rows[2]).tobytes()
    assert got["cnt"].max() <= 16
    applied = got["feat_root"].copy()
    live = np.arange(16)[None, :] < got["cnt"][:, None]
    r, k = np.nonzero(live)
    col = got["col"][r, k]
    assert (col >= 0).all() and (col < 198).all()
    # the old values are the root's, no listed column is unchanged, none is listed twice
    assert np.array_equal(got["oldv"][r, k].view(np.uint32), got["feat_root"][r, col].view(np.uint32))
    assert (got["oldv"][r, k] != got["newv"][r, k]).all()
    assert len(np.unique(r.astype(np.int64) * 198 + col)) == len(r)
    assert (np.diff(np.where(live, got["col"], 1000), axis=1)[live[:, 1:]] > 0).all()  # ascending
    applied[r, col] = got["newv"][r, k]
    assert np.array_equal(applied.view(np.uint32), got["feat_row"].view(np.uint32))
    # a record's own list: its non-zero columns, ascending
    for i in range(0, n, max(1, n // 4000)):
        nz = np.nonzero(got["feat_root"][i])[0]
        assert got["nz_cnt"][i] == len(nz)
        assert np.array_equal(got["nz_col"][i, :len(nz)], nz)
        assert np.array_equal(got["nz_val"][i, :len(nz)].view(np.uint32), got["feat_root"][i, nz].view(np.uint32))
    assert got["nz_cnt"].max() <= 33


def test_column_deltas_are_exact_ref2(hc, ref2_case):
    rows, ref = ref2_case
    assert len(rows[6]) == 37534 and int((rows[6] != 0).sum()) == 181
    assert (rows[5][rows[6] != 0] == 1).any() and (rows[5][rows[6] != 0] == -1).any()  # both colours win
    got = host_lists(hc, rows)
    check_lists(got, rows, ref)
    live = rows[6] == 0
    assert got["cnt"][live].max() == 6  # four moved-checker columns and the player one-hot
    assert 5.4 < got["cnt"][live].mean() < 5.6


def test_column_deltas_are_exact_full4(hc, full4_case):
    rows, ref = full4_case
    assert len(rows[6]) == 19592 + R.BIG_ROWS
    got = host_lists(hc, rows)
    check_lists(got, rows, ref)
    # a point changes by 2..4 on some rows: its count's change spans several columns
    change = np.abs(rows[3].astype(np.int32) - rows[0].astype(np.int32)).max(1)
    assert {2, 3, 4} <= set(np.unique(change))
    assert got["cnt"].max() <= hc.hc_value_slots()  # what a row's list holds


def host_values(hc, rows, net, perspective):
    n = len(rows[6])
    w1t = np.ascontiguousarray(net.l1.weight.detach().numpy().T, dtype=np.float32)
    b1 = np.ascontiguousarray(net.l1.bias.detach().numpy(), dtype=np.float32)
    w2 = np.ascontiguousarray(net.l2.weight.detach().numpy().reshape(-1), dtype=np.float32)
    b2 = np.ascontiguousarray(net.l2.bias.detach().numpy(), dtype=np.float32)
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    value = np.full(n, np.nan, np.float32)
    hc.hc_value_rows(ctypes.c_int64(n), *(P(a) for a in rows), P(w1t), ctypes.c_int64(w1t.shape[1]), P(b1), P(w2),
                     P(b2), net.hidden, HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act],
                     1 if perspective == "white" else 0, P(value))
    return value


@pytest.mark.parametrize("spec", NETS, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_values_through_the_shared_arithmetic(hc, ref2_case, full4_case, spec):
    net = make_net(*spec)
    for name, (rows, ref) in (("ref2", ref2_case), ("full4", full4_case)):
        want, E = torch_values(net, ref["feat"])
        tol = TOL_FACTOR * E
        live = rows[6] == 0
        assert E > 0 and np.ptp(want[live]) > 1e3 * tol  # the values differ: a wrong column would show
        for perspective in ("white", "mover"):
            got = host_values(hc, rows, net, perspective)
            err = float(np.abs(got[live].astype(np.float64) - want[live]).max())
            print(f"{name} {spec[:3]} {perspective}: E = {E:.3e}, max error = {err:.3e} = {err / E:.2f} E")
            assert err <= tol, (name, perspective, err, tol)
            assert np.array_equal(got[~live], outcome(rows[6][~live], rows[5][~live], perspective))
        assert (~live).any() or name == "full4"
