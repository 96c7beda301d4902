"""narde_net_table, narde_value_rollout_league, narde_turn_value_rollout_league:
exported, bound, and their arguments validated before any device call
(CPU-safe: no GPU is touched -- a call that reached the device would return
NARDE_EHIP here)."""
import ctypes

import pytest

from gym_narde import _lib

EINVAL = -1
N = None


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("narde_net_table", 6), ("narde_value_rollout_league", 17),
                        ("narde_turn_value_rollout_league", 19)):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.LEAGUE_NETS_MAX == 64 and _lib.league_table_bytes(3) == 192


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=1)
    f.update(kw)
    return _lib.ValueMlp(**f)


@pytest.fixture(scope="module")
def mem():
    """Stand-ins for a handle and for device arrays: the argument checks
    return before they read them."""
    raw = ctypes.create_string_buffer(64 * 64 + 512 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    h = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    return dict(raw=raw, h=h, buf=ctypes.c_void_p(base), odd2=ctypes.c_void_p(base + 2),
                odd4=ctypes.c_void_p(base + 4), odd8=ctypes.c_void_p(base + 8))


BAD_NETS = {
    "NULL w1t": dict(w1t=N), "NULL b1": dict(b1=N), "NULL w2": dict(w2=N), "NULL b2": dict(b2=N),
    "hidden 0": dict(hidden=0), "hidden 129": dict(hidden=129, ld_w1t=129), "ld_w1t < hidden": dict(ld_w1t=79),
    "ld_w1t too large": dict(ld_w1t=(1 << 20) + 1), "hidden_act 3": dict(hidden_act=3),
    "hidden_act -1": dict(hidden_act=-1), "out_act 3": dict(out_act=3), "out_act -1": dict(out_act=-1),
}


def test_net_table_argument_errors(mem):
    lib = _lib.load()
    fn = lib.narde_net_table
    buf, odd4 = mem["buf"], mem["odd4"]
    nets = (_lib.ValueMlp * 64)(*[_net(buf) for _ in range(64)])
    #        device n_nets nets table table_bytes stream
    cases = {
        "negative device": (-1, 3, nets, buf, 192, N),
        "NULL nets": (0, 3, N, buf, 192, N),
        "NULL table": (0, 3, nets, N, 192, N),
        "n_nets 0": (0, 0, nets, buf, 4096, N),
        "n_nets -1": (0, -1, nets, buf, 4096, N),
        "n_nets 65": (0, 65, nets, buf, 65 * 64, N),
        "misaligned table": (0, 3, nets, odd4, 192, N),
        "table_bytes one short": (0, 3, nets, buf, 191, N),
        "table_bytes negative": (0, 3, nets, buf, -1, N),
        "table_bytes of 63 nets for 64": (0, 64, nets, buf, 63 * 64, N),
    }
    for what, args in cases.items():
        rc = fn(*args)
        assert rc == EINVAL, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
    for what, kw in BAD_NETS.items():  # any net's error, wherever it stands
        for at, n in ((0, 1), (2, 3), (63, 64)):
            arr = (_lib.ValueMlp * n)(*[_net(buf, **(kw if i == at else {})) for i in range(n)])
            rc = fn(0, n, arr, buf, 64 * n, N)
            assert rc == EINVAL, f"{what} at {at} of {n} returned {rc}"
            assert f"net {at}:".encode() in lib.narde_last_error(), (what, at, lib.narde_last_error())


def test_net_table_names_the_bad_net_at_index_2_of_3(mem):
    lib = _lib.load()
    buf = mem["buf"]
    arr = (_lib.ValueMlp * 3)(_net(buf), _net(buf), _net(buf, hidden=0))
    assert lib.narde_net_table(0, 3, arr, buf, 192, N) == EINVAL
    msg = lib.narde_last_error()
    assert b"net 2" in msg and b"hidden" in msg, msg


def _league_cases(h, buf, odd2, odd_col, tail):
    """The cases the two league rollouts share; odd_col: a misaligned action
    column; tail: the arguments behind truncated."""
    #        env plies table n_nets white black eps seed tag dice column value reward term trunc ...
    outs = (N, N, N, N, N, N)
    return {
        "NULL handle": (N, 1, buf, 3, buf, buf, N, 0, N, *outs, *tail),
        "plies 0": (h, 0, buf, 3, buf, buf, N, 0, N, *outs, *tail),
        "plies -1": (h, -1, buf, 3, buf, buf, N, 0, N, *outs, *tail),
        "NULL table": (h, 1, N, 3, buf, buf, N, 0, N, *outs, *tail),
        "NULL white": (h, 1, buf, 3, N, buf, N, 0, N, *outs, *tail),
        "NULL black": (h, 1, buf, 3, buf, N, N, 0, N, *outs, *tail),
        "misaligned table": (h, 1, ctypes.c_void_p(buf.value + 8), 3, buf, buf, N, 0, N, *outs, *tail),
        "misaligned white": (h, 1, buf, 3, odd2, buf, N, 0, N, *outs, *tail),
        "misaligned black": (h, 1, buf, 3, buf, odd2, N, 0, N, *outs, *tail),
        "n_nets 0": (h, 1, buf, 0, buf, buf, N, 0, N, *outs, *tail),
        "n_nets -1": (h, 1, buf, -1, buf, buf, N, 0, N, *outs, *tail),
        "n_nets 65": (h, 1, buf, 65, buf, buf, N, 0, N, *outs, *tail),
        "epsilon without tag": (h, 1, buf, 3, buf, buf, buf, 0, N, *outs, *tail),
        "tag without epsilon": (h, 1, buf, 3, buf, buf, N, 0, buf, *outs, *tail),
        "misaligned column": (h, 1, buf, 3, buf, buf, N, 0, N, N, odd_col, N, N, N, N, *tail),
    }


def test_value_rollout_league_argument_errors(mem):
    lib = _lib.load()
    fn = lib.narde_value_rollout_league
    h, buf, odd2, odd8 = mem["h"], mem["buf"], mem["odd2"], mem["odd8"]
    cases = _league_cases(h, buf, odd2, odd2, (N, N))  # records, stream
    cases["misaligned records"] = (h, 1, buf, 3, buf, buf, N, 0, N, N, N, N, N, N, N, odd8, N)
    for what, args in cases.items():
        rc = fn(*args)
        assert rc == EINVAL, f"{what} returned {rc}"
        assert lib.narde_last_error(), what


def test_turn_value_rollout_league_argument_errors(mem):
    lib = _lib.load()
    fn = lib.narde_turn_value_rollout_league
    h, buf, odd2, odd4, odd8 = mem["h"], mem["buf"], mem["odd2"], mem["odd4"], mem["odd8"]
    piece = _lib.turn_rollout_scratch_bytes(1)
    cases = _league_cases(h, buf, odd2, odd4, (buf, piece, N, N))  # scratch, scratch_bytes, records, stream
    outs = (N, N, N, N, N, N)
    cases.update({
        "misaligned records": (h, 1, buf, 3, buf, buf, N, 0, N, *outs, buf, piece, odd8, N),
        "NULL scratch": (h, 1, buf, 3, buf, buf, N, 0, N, *outs, N, piece, N, N),
        "misaligned scratch": (h, 1, buf, 3, buf, buf, N, 0, N, *outs, odd8, piece, N, N),
        "scratch_bytes below a piece": (h, 1, buf, 3, buf, buf, N, 0, N, *outs, buf, piece - 1, N, N),
        "scratch_bytes negative": (h, 1, buf, 3, buf, buf, N, 0, N, *outs, buf, -1, N, N),
    })
    for what, args in cases.items():
        rc = fn(*args)
        assert rc == EINVAL, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
