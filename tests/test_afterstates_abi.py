"""narde_afterstates / narde_afterstate_pick: exported, bound, and their
arguments validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes

from gym_narde import _lib


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("narde_afterstates", "narde_afterstate_pick"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["narde_afterstates"][1]) == 10
    assert len(_lib.SIGNATURES["narde_afterstate_pick"][1]) == 13


def test_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    # a stand-in for a handle: the argument checks return before they read it
    h = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(512), ctypes.c_void_p)
    cases = [
        ("narde_afterstates", (N, N, 0, buf, N, N, N, N, N, N)),       # NULL handle
        ("narde_afterstates", (h, N, 0, N, N, N, N, N, N, N)),         # NULL offsets
        ("narde_afterstates", (h, N, -1, buf, N, N, N, N, N, N)),      # negative cap
        ("narde_afterstate_pick", (N, buf, buf, 4, buf, 1, 1, N, 0, N, buf, N, N)),   # NULL handle
        ("narde_afterstate_pick", (h, N, buf, 4, buf, 1, 1, N, 0, N, buf, N, N)),     # NULL offsets
        ("narde_afterstate_pick", (h, buf, N, 4, buf, 1, 1, N, 0, N, buf, N, N)),     # NULL codes
        ("narde_afterstate_pick", (h, buf, buf, 4, N, 1, 1, N, 0, N, buf, N, N)),     # NULL values
        ("narde_afterstate_pick", (h, buf, buf, 4, buf, 1, 1, N, 0, N, N, N, N)),     # NULL actions
        ("narde_afterstate_pick", (h, buf, buf, -1, buf, 1, 1, N, 0, N, buf, N, N)),  # negative cap
        ("narde_afterstate_pick", (h, buf, buf, 4, buf, 1, 2, N, 0, N, buf, N, N)),   # perspective
        ("narde_afterstate_pick", (h, buf, buf, 4, buf, 1, -1, N, 0, N, buf, N, N)),
        ("narde_afterstate_pick", (h, buf, buf, 4, buf, 0, 1, N, 0, N, buf, N, N)),   # ld_value < 1
        ("narde_afterstate_pick", (h, buf, buf, 4, buf, 1, 1, buf, 0, N, buf, N, N)),  # epsilon without a tag
    ]
    for name, args in cases:
        rc = getattr(lib, name)(*args)
        assert rc == -1, f"{name}{args} returned {rc}"
        assert lib.narde_last_error(), name
