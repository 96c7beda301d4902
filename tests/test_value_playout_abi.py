"""narde_state_records, narde_value_playout and narde_turn_value_playout:
exported, bound, and their arguments validated before any device call
(CPU-safe: no GPU is touched)."""
import ctypes
import struct

from gym_narde import _lib

B = 100


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("narde_state_records", 9), ("narde_value_playout", 15), ("narde_turn_value_playout", 17)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    # the FULL4 call: the REF2 call's arguments, then scratch and its size ahead of the stream
    a, b = _lib.SIGNATURES["narde_value_playout"][1], _lib.SIGNATURES["narde_turn_value_playout"][1]
    assert b[:len(a) - 1] == a[:-1] and b[-3:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert a[1] is ctypes.c_int64 and a[7] is ctypes.c_uint64 and a[8] is ctypes.c_int64
    assert _lib.SIGNATURES["narde_state_records"][1][:2] == [ctypes.c_int, ctypes.c_int64]
    assert _lib.SIGNATURES["narde_state_records"][1][6] is ctypes.c_uint32
    assert _lib.PLAYOUT_COMMON_DICE == 1


def _aligned(nbytes):
    """(keep-alive, a 16-B aligned address inside it)"""
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)


def _handle():
    # a stand-in for a handle: the checks read its fields and return before any launch
    hraw = ctypes.create_string_buffer(512)
    struct.pack_into("q", hraw, 8, B)
    return hraw, ctypes.cast(hraw, ctypes.c_void_p)


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=2)
    f.update(kw)
    return _lib.ValueMlp(**f)


def _cases(full):
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    hraw, h = _handle()
    R = ctypes.byref
    ok = _net(buf)
    piece = _lib.turn_rollout_scratch_bytes(1)

    def call(handle=h, n=3, roots=buf, trials=4, max_plies=5, w=R(ok), b=R(ok), id_base=0, flags=0, sums=buf,
             scratch=buf, nbytes=piece):
        args = (handle, n, roots, trials, max_plies, w, b, 7, id_base, flags, sums, N, N, N)
        return args + ((scratch, nbytes, N) if full else (N,))

    cases = {
        "NULL handle": call(handle=N),
        "NULL roots": call(roots=N),
        "NULL sums": call(sums=N),
        "both nets NULL": call(w=N, b=N),
        "NULL w1t": call(w=R(_net(buf, w1t=N))),
        "NULL b1": call(b=R(_net(buf, b1=N)), w=N),
        "NULL w2": call(w=R(_net(buf, w2=N))),
        "NULL b2": call(w=R(_net(buf, b2=N))),
        "hidden 0": call(w=R(_net(buf, hidden=0))),
        "hidden 129": call(b=R(_net(buf, hidden=129, ld_w1t=129))),
        "ld_w1t < hidden": call(w=R(_net(buf, ld_w1t=79))),
        "hidden_act 3": call(w=R(_net(buf, hidden_act=3))),
        "out_act -1": call(b=R(_net(buf, out_act=-1))),
        "n 0": call(n=0),
        "n -1": call(n=-1),
        "trials 0": call(trials=0),
        "trials -2": call(trials=-2),
        "max_plies 0": call(max_plies=0),
        "max_plies -1": call(max_plies=-1),
        "n x trials 2^31": call(n=2 ** 20, trials=2 ** 11),
        "n 2^31": call(n=2 ** 31, trials=1),
        "trials x max_plies 2^31": call(n=1, trials=2 ** 16, max_plies=2 ** 15),
        "unknown flag 2": call(flags=2),
        "unknown flag 3": call(flags=3),
        "unknown flag -1": call(flags=-1),
        "roots misaligned": call(roots=odd),
        "id_base -1": call(id_base=-1),
        "id_base + n x trials 2^32": call(id_base=2 ** 32 - 12),
    }
    if full:
        cases.update({"NULL scratch": call(scratch=N), "scratch misaligned": call(scratch=odd),
                      "scratch below one piece": call(nbytes=piece - 1), "scratch 0": call(nbytes=0)})
    return (keep, hraw), cases


def test_playout_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    for name, full in (("narde_value_playout", False), ("narde_turn_value_playout", True)):
        fn = getattr(lib, name)
        keep, cases = _cases(full)
        for what, args in cases.items():
            lib.narde_version()
            rc = fn(*args)
            assert rc == -1, f"{name}: {what} returned {rc}"
            assert lib.narde_last_error(), what
        # the messages name what is wrong
        words = [("max_plies 0", b"max_plies"), ("trials 0", b"trials"), ("roots misaligned", b"roots"),
                 ("unknown flag 2", b"flag"), ("id_base -1", b"id_base"), ("id_base + n x trials 2^32", b"id_base"),
                 ("n x trials 2^31", b"n x trials"), ("trials x max_plies 2^31", b"trials x max_plies")]
        if full:
            words += [("scratch misaligned", b"scratch"), ("scratch below one piece", b"NARDE_TURN_ROLLOUT_SCRATCH_BYTES")]
        for what, word in words:
            assert fn(*cases[what]) == -1 and word in lib.narde_last_error(), (name, what)
        del keep


def test_state_records_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    N = None

    def call(n=3, board=buf, off=buf, ft=buf, player=buf, records=buf):
        return (0, n, board, off, ft, player, 0, records, N)

    cases = {"NULL board": call(board=N), "NULL off": call(off=N), "NULL first_turn": call(ft=N),
             "NULL player": call(player=N), "NULL records": call(records=N), "n 0": call(n=0), "n -1": call(n=-1),
             "n 2^31": call(n=2 ** 31), "records misaligned": call(records=odd)}
    for what, args in cases.items():
        lib.narde_version()
        assert lib.narde_state_records(*args) == -1, what
        assert lib.narde_last_error(), what
    assert lib.narde_state_records(*cases["records misaligned"]) == -1 and b"records" in lib.narde_last_error()
    del keep
