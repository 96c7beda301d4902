"""narde_afterstates_records, narde_turn_afterstates_records, narde_rows_topk,
narde_playout_pick and narde_turn_playout_pick: exported, bound, and their
arguments validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes
import struct

from gym_narde import _lib

B = 100
NEW = (("narde_afterstates_records", 12), ("narde_turn_afterstates_records", 12), ("narde_rows_topk", 11),
       ("narde_playout_pick", 15), ("narde_turn_playout_pick", 15))


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW:
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    # the records calls: the scored calls' arguments with records ahead of the stream
    for kind in ("narde_afterstates", "narde_turn_afterstates"):
        a, b = _lib.SIGNATURES[kind + "_scored"][1], _lib.SIGNATURES[kind + "_records"][1]
        assert b[:len(a) - 1] == a[:-1] and b[-2:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["narde_playout_pick"] == _lib.SIGNATURES["narde_turn_playout_pick"]
    t = _lib.SIGNATURES["narde_rows_topk"][1]
    assert t[2] is ctypes.c_int64 and t[4] is ctypes.c_int64 and t[5] is ctypes.c_int and t[6] is ctypes.c_int
    assert _lib.TOPK_MAX == 64 and _lib.RECORD_NONE_WORD6 == 0xFF and _lib.PLAYOUT_COMMON_DICE == 1


def test_header_states_the_constants():
    import os

    text = open(os.path.join(os.path.dirname(_lib.HERE), "..", "include", "narde.h")).read()
    assert "#define NARDE_TOPK_MAX 64" in text
    assert "#define NARDE_RECORD_NONE_WORD6 0xFFu" in text
    for name, _ in NEW:
        assert f"int {name}(" in text, name


def _aligned(nbytes):
    """(keep-alive, a 16-B aligned address inside it)"""
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)


def _handle(n=B):
    # a stand-in for a handle: the checks read its fields and return before any launch
    hraw = ctypes.create_string_buffer(512)
    struct.pack_into("q", hraw, 8, n)
    return hraw, ctypes.cast(hraw, ctypes.c_void_p)


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=2)
    f.update(kw)
    return _lib.ValueMlp(**f)


def _all_einval(fn, cases, name):
    lib = _lib.load()
    for what, args in cases.items():
        lib.narde_version()
        rc = fn(*args)
        assert rc == -1, f"{name}: {what} returned {rc}"
        assert lib.narde_last_error(), what


def test_records_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    keep, buf = _aligned(512)
    odd4 = ctypes.c_void_p(buf.value + 4)
    odd2 = ctypes.c_void_p(buf.value + 2)
    hraw, h = _handle()
    big_raw, big = _handle(2 ** 31 // 1152 + 1)  # B x rows-per-env reaches 2^31 for either kind
    R = ctypes.byref
    ok = _net(buf)
    for name in ("narde_afterstates_records", "narde_turn_afterstates_records"):

        def call(handle=h, cap=8, offsets=buf, column=buf, net=R(ok), perspective=1, value=buf, records=buf):
            return (handle, N, cap, offsets, buf, column, buf, net, perspective, value, records, N)

        cases = {
            # the scored call's cases
            "NULL handle": call(handle=N),
            "NULL offsets": call(offsets=N),
            "cap -1": call(cap=-1),
            "too many envs": call(handle=big),
            "column misaligned": call(column=odd2),
            "perspective 2": call(perspective=2),
            "perspective -1": call(perspective=-1),
            "NULL w1t": call(net=R(_net(buf, w1t=N))),
            "hidden 0": call(net=R(_net(buf, hidden=0))),
            "hidden 129": call(net=R(_net(buf, hidden=129, ld_w1t=129))),
            "ld_w1t < hidden": call(net=R(_net(buf, ld_w1t=79))),
            "hidden_act 3": call(net=R(_net(buf, hidden_act=3))),
            "out_act -1": call(net=R(_net(buf, out_act=-1))),
            # its own
            "NULL records": call(records=N),
            "NULL records, no net": call(records=N, net=N, value=N),
            "records misaligned": call(records=odd4),
            "records misaligned, no net": call(records=odd4, net=N, value=N),
            "net without value": call(value=N),
            "value without net": call(net=N),
        }
        fn = getattr(lib, name)
        _all_einval(fn, cases, name)
        for what, word in (("NULL records", b"records"), ("records misaligned", b"records"),
                           ("net without value", b"net and value"), ("value without net", b"net and value"),
                           ("cap -1", b"cap")):
            assert fn(*cases[what]) == -1 and word in lib.narde_last_error(), (name, what)
    del keep, hraw, big_raw


def test_topk_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    hraw, h = _handle()
    big_raw, big = _handle(2 ** 31 // 64)  # B x k = 2^31 at k = 64

    def call(handle=h, offsets=buf, cap=8, value=buf, ld=1, perspective=1, k=4, records=buf, sel=buf, roots=buf):
        return (handle, offsets, cap, value, ld, perspective, k, records, sel, roots, N)

    cases = {
        "NULL handle": call(handle=N),
        "NULL offsets": call(offsets=N),
        "NULL value": call(value=N),
        "NULL sel": call(sel=N),
        "k 0": call(k=0),
        "k -1": call(k=-1),
        "k 65": call(k=65),
        "perspective 2": call(perspective=2),
        "perspective -1": call(perspective=-1),
        "cap -1": call(cap=-1),
        "ld 0": call(ld=0),
        "roots without records": call(records=N),
        "records without roots": call(roots=N),
        "roots misaligned": call(roots=odd),
        "records misaligned": call(records=odd),
        "B x k 2^31": call(handle=big, k=64),
    }
    _all_einval(lib.narde_rows_topk, cases, "narde_rows_topk")
    for what, word in (("k 65", b"NARDE_TOPK_MAX"), ("perspective 2", b"perspective"), ("cap -1", b"cap"),
                       ("roots without records", b"roots and records"), ("roots misaligned", b"16-B"),
                       ("B x k 2^31", b"B x k")):
        assert lib.narde_rows_topk(*cases[what]) == -1 and word in lib.narde_last_error(), what
    del keep, hraw, big_raw


def test_playout_pick_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    keep, buf = _aligned(512)
    hraw, h = _handle()
    for name, align in (("narde_playout_pick", 4), ("narde_turn_playout_pick", 8)):
        odd = ctypes.c_void_p(buf.value + align // 2)

        def call(handle=h, k=4, sel=buf, cap=8, value=buf, ld=1, reward=buf, column=buf, trials=4, sums=buf, out=buf):
            return (handle, k, sel, cap, value, ld, reward, column, trials, sums, N, out, N, N, N)

        cases = {
            "NULL handle": call(handle=N),
            "NULL sel": call(sel=N),
            "NULL value": call(value=N),
            "NULL reward": call(reward=N),
            "NULL sums": call(sums=N),
            "NULL column": call(column=N),
            "NULL out": call(out=N),
            "k 0": call(k=0),
            "k 65": call(k=65),
            "k -3": call(k=-3),
            "trials 0": call(trials=0),
            "trials -1": call(trials=-1),
            "cap -1": call(cap=-1),
            "ld 0": call(ld=0),
            "B x k x trials 2^31": call(k=64, trials=2 ** 31 // (64 * B) + 1),
            "column misaligned": call(column=odd),
            "out misaligned": call(out=odd),
        }
        fn = getattr(lib, name)
        _all_einval(fn, cases, name)
        for what, word in (("k 65", b"NARDE_TOPK_MAX"), ("trials 0", b"trials"),
                           ("B x k x trials 2^31", b"B x k x trials"), ("column misaligned", b"aligned")):
            assert fn(*cases[what]) == -1 and word in lib.narde_last_error(), (name, what)
    del keep, hraw
