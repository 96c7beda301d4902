"""narde_turn_afterstates_lookahead: exported, bound, and its arguments
validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes

from gym_narde import _lib

NAME = "narde_turn_afterstates_lookahead"


def test_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 13
    # 128 B a row: the record, the rolls' bests, the rolls to redo; linear in cap
    assert _lib.turn_lookahead_scratch_bytes(0) == 0 and _lib.turn_lookahead_scratch_bytes(7) == 896


def test_the_row_kinds_name_their_scratch():
    from gym_narde import vector

    assert vector._FULL4_ROWS.look_scratch(3) == 384 and vector._REF2_ROWS.look_scratch(3) == 96
    assert vector._FULL4_ROWS.expand + "_lookahead" == NAME


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
    raw = ctypes.create_string_buffer(1024 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    buf = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 8)  # 8-B but not 16-B aligned
    odd4 = ctypes.c_void_p(base + 4)  # 4-B but not 8-B aligned
    ok = _net(buf)
    R = ctypes.byref
    cases = {
        # everything narde_turn_afterstates_scored rejects
        "NULL handle": (N, N, 4, buf, N, N, N, R(ok), 1, buf, buf, 512, N),
        "NULL offsets": (h, N, 4, N, N, N, N, R(ok), 1, buf, buf, 512, N),
        "negative cap": (h, N, -1, buf, N, N, N, R(ok), 1, buf, buf, 512, N),
        "misaligned play": (h, N, 4, buf, N, odd4, N, R(ok), 1, buf, buf, 512, N),
        "NULL net": (h, N, 4, buf, N, N, N, N, 1, buf, buf, 512, N),
        "NULL value": (h, N, 4, buf, N, N, N, R(ok), 1, N, buf, 512, N),
        "NULL w1t": (h, N, 4, buf, N, N, N, R(_net(buf, w1t=N)), 1, buf, buf, 512, N),
        "NULL b2": (h, N, 4, buf, N, N, N, R(_net(buf, b2=N)), 1, buf, buf, 512, N),
        "hidden 0": (h, N, 4, buf, N, N, N, R(_net(buf, hidden=0)), 1, buf, buf, 512, N),
        "hidden 129": (h, N, 4, buf, N, N, N, R(_net(buf, hidden=129, ld_w1t=129)), 1, buf, buf, 512, N),
        "ld_w1t < hidden": (h, N, 4, buf, N, N, N, R(_net(buf, ld_w1t=79)), 1, buf, buf, 512, N),
        "hidden_act 3": (h, N, 4, buf, N, N, N, R(_net(buf, hidden_act=3)), 1, buf, buf, 512, N),
        "hidden_act -1": (h, N, 4, buf, N, N, N, R(_net(buf, hidden_act=-1)), 1, buf, buf, 512, N),
        "out_act 3": (h, N, 4, buf, N, N, N, R(_net(buf, out_act=3)), 1, buf, buf, 512, N),
        "perspective 2": (h, N, 4, buf, N, N, N, R(ok), 2, buf, buf, 512, N),
        "perspective -1": (h, N, 4, buf, N, N, N, R(ok), -1, buf, buf, 512, N),
        # the lookahead's own rules
        "perspective 0 (the mover's)": (h, N, 4, buf, N, N, N, R(ok), 0, buf, buf, 512, N),
        "NULL scratch": (h, N, 4, buf, N, N, N, R(ok), 1, buf, N, 512, N),
        "scratch one byte short": (h, N, 4, buf, N, N, N, R(ok), 1, buf, buf, 511, N),
        "scratch sized for the REF2 call": (h, N, 4, buf, N, N, N, R(ok), 1, buf, buf, 128, N),
        "scratch_bytes 0": (h, N, 4, buf, N, N, N, R(ok), 1, buf, buf, 0, N),
        "negative scratch_bytes": (h, N, 4, buf, N, N, N, R(ok), 1, buf, buf, -1, N),
        "misaligned scratch": (h, N, 4, buf, N, N, N, R(ok), 1, buf, odd, 1024, N),
    }
    for what, args in cases.items():
        rc = fn(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
