"""narde_turn_value_rollout and narde_turn_value_rollout_waves: exported,
bound, and their arguments validated before any device call (CPU-safe: no GPU
is touched)."""
import ctypes

from gym_narde import _lib

NAME = "narde_turn_value_rollout"
WAVES = "narde_turn_value_rollout_waves"
PIECE = 83536


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME) and hasattr(lib, WAVES)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 16
    assert WAVES in _lib.SIGNATURES and len(_lib.SIGNATURES[WAVES][1]) == 2
    assert _lib.turn_rollout_scratch_bytes(3) == 3 * PIECE


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=1)
    f.update(kw)
    return _lib.ValueMlp(**f)


def test_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    N = None
    # stand-ins for a handle and for device arrays: the argument checks return before they read them
    h = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    raw = ctypes.create_string_buffer(512 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    buf = ctypes.c_void_p(base)
    odd4 = ctypes.c_void_p(base + 4)
    odd8 = ctypes.c_void_p(base + 8)
    ok = _net(buf)
    R = ctypes.byref
    bad_nets = {
        "NULL w1t": _net(buf, w1t=N), "NULL b1": _net(buf, b1=N), "NULL w2": _net(buf, w2=N), "NULL b2": _net(buf, b2=N),
        "hidden 0": _net(buf, hidden=0), "hidden 129": _net(buf, hidden=129, ld_w1t=129),
        "ld_w1t < hidden": _net(buf, ld_w1t=79), "ld_w1t too large": _net(buf, ld_w1t=(1 << 20) + 1),
        "hidden_act 3": _net(buf, hidden_act=3), "hidden_act -1": _net(buf, hidden_act=-1),
        "out_act 3": _net(buf, out_act=3), "out_act -1": _net(buf, out_act=-1),
    }
    #        env plies white black eps seed tag dice play value reward term trunc scratch bytes stream
    cases = {
        "NULL handle": (N, 1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, buf, PIECE, N),
        "plies 0": (h, 0, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, buf, PIECE, N),
        "plies -1": (h, -1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, buf, PIECE, N),
        "both nets NULL": (h, 1, N, N, N, 0, N, N, N, N, N, N, N, buf, PIECE, N),
        "epsilon without tag": (h, 1, R(ok), R(ok), buf, 0, N, N, N, N, N, N, N, buf, PIECE, N),
        "tag without epsilon": (h, 1, R(ok), R(ok), N, 0, buf, N, N, N, N, N, N, buf, PIECE, N),
        "misaligned play": (h, 1, R(ok), R(ok), N, 0, N, N, odd4, N, N, N, N, buf, PIECE, N),
        "NULL scratch": (h, 1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, N, PIECE, N),
        "misaligned scratch": (h, 1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, odd8, PIECE, N),
        "scratch one byte short": (h, 1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, buf, PIECE - 1, N),
        "scratch_bytes 0": (h, 1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, buf, 0, N),
        "scratch_bytes negative": (h, 1, R(ok), R(ok), N, 0, N, N, N, N, N, N, N, buf, -PIECE, N),
    }
    for what, net in bad_nets.items():  # narde_value_rollout's net errors, for either net
        cases[f"white: {what}"] = (h, 1, R(net), R(ok), N, 0, N, N, N, N, N, N, N, buf, PIECE, N)
        cases[f"black: {what}"] = (h, 1, R(ok), R(net), N, 0, N, N, N, N, N, N, N, buf, PIECE, N)
        cases[f"white alone: {what}"] = (h, 1, R(net), N, N, 0, N, N, N, N, N, N, N, buf, PIECE, N)
        cases[f"black alone: {what}"] = (h, 1, N, R(net), N, 0, N, N, N, N, N, N, N, buf, PIECE, N)
    for what, args in cases.items():
        rc = fn(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what


def test_waves_query_rejects_null_arguments():
    lib = _lib.load()
    fn = getattr(lib, WAVES)
    h = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    w = ctypes.c_int(0)
    for what, args in {"NULL handle": (None, ctypes.byref(w)), "NULL waves": (h, None), "both NULL": (None, None)}.items():
        rc = fn(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
