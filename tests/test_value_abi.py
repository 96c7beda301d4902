"""narde_afterstates_scored / narde_turn_afterstates_scored: exported, bound,
and their arguments validated before any device call (CPU-safe: no GPU is
touched)."""
import ctypes

import pytest

from gym_narde import _lib

NAMES = ("narde_afterstates_scored", "narde_turn_afterstates_scored")


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == 11
    assert ctypes.sizeof(_lib.ValueMlp) == 56  # narde_value_mlp: 5 x 8 B, 3 x int32, padded to 8


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=1)
    f.update(kw)
    return _lib.ValueMlp(**f)


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_are_einval_before_any_device_call(name):
    lib = _lib.load()
    N = None
    # stand-ins for a handle and for device arrays: the argument checks return before they read them
    h = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    ok = _net(buf)
    R = ctypes.byref
    cases = {
        "NULL handle": (N, N, 4, buf, N, N, N, R(ok), 1, buf, N),
        "NULL offsets": (h, N, 4, N, N, N, N, R(ok), 1, buf, N),
        "negative cap": (h, N, -1, buf, N, N, N, R(ok), 1, buf, N),
        "NULL net": (h, N, 4, buf, N, N, N, N, 1, buf, N),
        "NULL value": (h, N, 4, buf, N, N, N, R(ok), 1, N, N),
        "NULL w1t": (h, N, 4, buf, N, N, N, R(_net(buf, w1t=N)), 1, buf, N),
        "NULL b2": (h, N, 4, buf, N, N, N, R(_net(buf, b2=N)), 1, buf, N),
        "hidden 0": (h, N, 4, buf, N, N, N, R(_net(buf, hidden=0)), 1, buf, N),
        "hidden 129": (h, N, 4, buf, N, N, N, R(_net(buf, hidden=129, ld_w1t=129)), 1, buf, N),
        "ld_w1t < hidden": (h, N, 4, buf, N, N, N, R(_net(buf, ld_w1t=79)), 1, buf, N),
        "hidden_act 3": (h, N, 4, buf, N, N, N, R(_net(buf, hidden_act=3)), 1, buf, N),
        "hidden_act -1": (h, N, 4, buf, N, N, N, R(_net(buf, hidden_act=-1)), 1, buf, N),
        "out_act 3": (h, N, 4, buf, N, N, N, R(_net(buf, out_act=3)), 1, buf, N),
        "perspective 2": (h, N, 4, buf, N, N, N, R(ok), 2, buf, N),
        "perspective -1": (h, N, 4, buf, N, N, N, R(ok), -1, buf, N),
    }
    for what, args in cases.items():
        rc = getattr(lib, name)(*args)
        assert rc == -1, f"{name}: {what} returned {rc}"
        assert lib.narde_last_error(), what
