"""narde_turn_afterstates / narde_turn_pick: exported, bound, and their
arguments validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes

from gym_narde import _lib


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("narde_turn_afterstates", "narde_turn_pick"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["narde_turn_afterstates"][1]) == 10
    assert len(_lib.SIGNATURES["narde_turn_pick"][1]) == 13


def test_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    # a stand-in for a handle: the argument checks return before they read it
    h = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    raw = ctypes.create_string_buffer(512 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    buf = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 4)  # 4-B aligned only
    cases = [
        ("narde_turn_afterstates", (N, N, 0, buf, N, N, N, N, N, N)),       # NULL handle
        ("narde_turn_afterstates", (h, N, 0, N, N, N, N, N, N, N)),         # NULL offsets
        ("narde_turn_afterstates", (h, N, -1, buf, N, N, N, N, N, N)),      # negative cap
        ("narde_turn_afterstates", (h, N, 4, buf, N, odd, N, N, N, N)),     # play not 8-B aligned
        ("narde_turn_afterstates", (h, N, 4, buf, N, N, odd, N, N, N)),     # feat not 16-B aligned
        ("narde_turn_afterstates", (h, N, 4, buf, N, N, N, odd, N, N)),     # obs not 16-B aligned
        ("narde_turn_pick", (N, buf, buf, 4, buf, 1, 1, N, 0, N, buf, N, N)),   # NULL handle
        ("narde_turn_pick", (h, N, buf, 4, buf, 1, 1, N, 0, N, buf, N, N)),     # NULL offsets
        ("narde_turn_pick", (h, buf, N, 4, buf, 1, 1, N, 0, N, buf, N, N)),     # NULL play
        ("narde_turn_pick", (h, buf, buf, 4, N, 1, 1, N, 0, N, buf, N, N)),     # NULL values
        ("narde_turn_pick", (h, buf, buf, 4, buf, 1, 1, N, 0, N, N, N, N)),     # NULL out_play
        ("narde_turn_pick", (h, buf, buf, -1, buf, 1, 1, N, 0, N, buf, N, N)),  # negative cap
        ("narde_turn_pick", (h, buf, buf, 4, buf, 1, 2, N, 0, N, buf, N, N)),   # perspective
        ("narde_turn_pick", (h, buf, buf, 4, buf, 1, -1, N, 0, N, buf, N, N)),
        ("narde_turn_pick", (h, buf, buf, 4, buf, 0, 1, N, 0, N, buf, N, N)),   # ld_value < 1
        ("narde_turn_pick", (h, buf, buf, 4, buf, 1, 1, buf, 0, N, buf, N, N)),  # epsilon without a tag
        ("narde_turn_pick", (h, buf, odd, 4, buf, 1, 1, N, 0, N, buf, N, N)),   # play not 8-B aligned
        ("narde_turn_pick", (h, buf, buf, 4, buf, 1, 1, N, 0, N, odd, N, N)),   # out_play not 8-B aligned
    ]
    for name, args in cases:
        rc = getattr(lib, name)(*args)
        assert rc == -1, f"{name}{args} returned {rc}"
        assert lib.narde_last_error(), name
