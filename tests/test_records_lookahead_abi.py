"""narde_records_lookahead, narde_turn_records_lookahead, narde_slot_pick and
narde_turn_slot_pick: exported, bound, and their arguments validated before
any device call (CPU-safe: no GPU is touched)."""
import ctypes

from gym_narde import _lib
from test_playout_pick_abi import B, _aligned, _all_einval, _handle, _net

NEW = (("narde_records_lookahead", 6), ("narde_turn_records_lookahead", 8), ("narde_slot_pick", 13),
       ("narde_turn_slot_pick", 13))


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW:
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    a, b = _lib.SIGNATURES["narde_records_lookahead"][1], _lib.SIGNATURES["narde_turn_records_lookahead"][1]
    # FULL4: the same arguments with the scratch and its size ahead of the stream
    assert b[:len(a) - 1] == a[:-1] and b[-3:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert a[1] is ctypes.c_int64 and a[3] == ctypes.POINTER(_lib.ValueMlp)
    assert _lib.SIGNATURES["narde_slot_pick"] == _lib.SIGNATURES["narde_turn_slot_pick"]
    # the playout pick's arguments less trials and sums, the leaf's place taken by the slot scores
    p, s = _lib.SIGNATURES["narde_playout_pick"][1], _lib.SIGNATURES["narde_slot_pick"][1]
    assert s == p[:8] + p[10:]


def test_header_declares_the_calls():
    import os

    text = open(os.path.join(os.path.dirname(_lib.HERE), "..", "include", "narde.h")).read()
    for name, _ in NEW:
        assert f"int {name}(" in text, name


def test_lookahead_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    keep, buf = _aligned(4096)
    odd = ctypes.c_void_p(buf.value + 4)
    hraw, h = _handle()
    R = ctypes.byref
    ok = _net(buf)
    for name, full in (("narde_records_lookahead", False), ("narde_turn_records_lookahead", True)):

        def call(handle=h, n=8, records=buf, net=R(ok), value=buf, scratch=buf, scratch_bytes=128 * 8):
            tail = (scratch, scratch_bytes, N) if full else (N,)
            return (handle, n, records, net, value) + tail

        cases = {
            "NULL handle": call(handle=N),
            "NULL records": call(records=N),
            "NULL net": call(net=N),
            "NULL value": call(value=N),
            "n 0": call(n=0),
            "n -1": call(n=-1),
            "n 2^31": call(n=2 ** 31, scratch_bytes=128 * 2 ** 31),
            "records misaligned": call(records=odd),
            # the scored call's net cases
            "NULL w1t": call(net=R(_net(buf, w1t=N))),
            "NULL b2": call(net=R(_net(buf, b2=N))),
            "hidden 0": call(net=R(_net(buf, hidden=0))),
            "hidden 129": call(net=R(_net(buf, hidden=129, ld_w1t=129))),
            "ld_w1t < hidden": call(net=R(_net(buf, ld_w1t=79))),
            "hidden_act 3": call(net=R(_net(buf, hidden_act=3))),
            "out_act -1": call(net=R(_net(buf, out_act=-1))),
        }
        if full:
            cases.update({
                "NULL scratch": call(scratch=N),
                "scratch misaligned": call(scratch=odd),
                "scratch one byte short": call(scratch_bytes=128 * 8 - 1),
                "scratch_bytes -1": call(scratch_bytes=-1),
            })
        fn = getattr(lib, name)
        _all_einval(fn, cases, name)
        words = [("n 0", b"n 0"), ("n 2^31", b"2^31"), ("records misaligned", b"records"), ("hidden 129", b"hidden")]
        if full:
            words += [("scratch one byte short", b"NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES"), ("scratch misaligned", b"scratch")]
        for what, word in words:
            assert fn(*cases[what]) == -1 and word in lib.narde_last_error(), (name, what)
    del keep, hraw


def test_slot_pick_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    N = None
    keep, buf = _aligned(512)
    hraw, h = _handle()
    big_raw, big = _handle(2 ** 31 // 64)  # B x k = 2^31 at k = 64
    for name, align in (("narde_slot_pick", 4), ("narde_turn_slot_pick", 8)):
        odd = ctypes.c_void_p(buf.value + align // 2)

        def call(handle=h, k=4, sel=buf, cap=8, value=buf, ld=1, reward=buf, column=buf, slot_score=buf, out=buf):
            return (handle, k, sel, cap, value, ld, reward, column, slot_score, out, N, N, N)

        cases = {
            "NULL handle": call(handle=N),
            "NULL sel": call(sel=N),
            "NULL value": call(value=N),
            "NULL reward": call(reward=N),
            "NULL slot_score": call(slot_score=N),
            "NULL column": call(column=N),
            "NULL out": call(out=N),
            "k 0": call(k=0),
            "k 65": call(k=65),
            "k -3": call(k=-3),
            "cap -1": call(cap=-1),
            "ld 0": call(ld=0),
            "B x k 2^31": call(handle=big, k=64),
            "column misaligned": call(column=odd),
            "out misaligned": call(out=odd),
        }
        fn = getattr(lib, name)
        _all_einval(fn, cases, name)
        for what, word in (("k 65", b"NARDE_TOPK_MAX"), ("cap -1", b"cap"), ("B x k 2^31", b"B x k"),
                           ("column misaligned", b"aligned")):
            assert fn(*cases[what]) == -1 and word in lib.narde_last_error(), (name, what)
    assert B == 100
    del keep, hraw, big_raw
