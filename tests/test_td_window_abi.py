"""narde_value_td_window and the records rollouts: exported, bound, and their
arguments validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes
import struct

from gym_narde import _lib

B = 100


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("narde_value_td_window", 14), ("narde_value_rollout_records", 15),
                        ("narde_turn_value_rollout_records", 17)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    # the parents with one more argument, ahead of the stream
    for parent in ("narde_value_rollout", "narde_turn_value_rollout"):
        a, b = _lib.SIGNATURES[parent][1], _lib.SIGNATURES[parent + "_records"][1]
        assert b[:len(a) - 1] == a[:-1] and len(b) == len(a) + 1
    assert _lib.TD_WINDOW_SLAB == 128
    assert _lib.td_window_scratch_floats(1, 1, 1) == 4 + 4 + 204
    assert _lib.td_window_scratch_floats(65, 7, 80) == 520 + 456 + 4 * 16004


def _aligned(nbytes):
    """(keep-alive, a 16-B aligned address inside it)"""
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)


def _handle():
    # a stand-in for a handle: the checks read its env count (an int64 behind
    # the device index) and return before any launch
    hraw = ctypes.create_string_buffer(512)
    struct.pack_into("q", hraw, 8, B)
    return hraw, ctypes.cast(hraw, ctypes.c_void_p)


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=2, w1=buf, ld_w1=198)
    f.update(kw)
    return _lib.ValueMlpTrain(**f)


def _window_cases():
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    hraw, h = _handle()
    R = ctypes.byref
    ok = _net(buf)
    need = _lib.td_window_scratch_floats(B, 3, 80)

    def call(handle=h, net=R(ok), plies=3, records=buf, reward=buf, term=buf, trunc=buf, lam=0.7, scratch=buf,
             floats=need, delta=N):
        return (handle, net, plies, records, reward, term, trunc, 0.1, lam, 1.0, scratch, floats, delta, N)

    cases = {
        "NULL handle": call(handle=N),
        "NULL net": call(net=N),
        "NULL w1t": call(net=R(_net(buf, w1t=N))),
        "NULL b1": call(net=R(_net(buf, b1=N))),
        "NULL w2": call(net=R(_net(buf, w2=N))),
        "NULL b2": call(net=R(_net(buf, b2=N))),
        "hidden 0": call(net=R(_net(buf, hidden=0))),
        "hidden 129": call(net=R(_net(buf, hidden=129, ld_w1t=129))),
        "ld_w1t < hidden": call(net=R(_net(buf, ld_w1t=79))),
        "ld_w1 < 198": call(net=R(_net(buf, ld_w1=197))),
        "hidden_act 3": call(net=R(_net(buf, hidden_act=3))),
        "out_act -1": call(net=R(_net(buf, out_act=-1))),
        "plies 0": call(plies=0, floats=10 ** 9),
        "plies -1": call(plies=-1, floats=10 ** 9),
        "plies past 2^31 samples": call(plies=2 ** 31 // B, floats=2 ** 62),
        "NULL records": call(records=N),
        "NULL reward": call(reward=N),
        "NULL terminated": call(term=N),
        "NULL truncated": call(trunc=N),
        "NULL scratch": call(scratch=N),
        "lam -0.1": call(lam=-0.1),
        "lam 1.5": call(lam=1.5),
        "lam NaN": call(lam=float("nan")),
        "records misaligned": call(records=odd),
        "scratch misaligned": call(scratch=odd),
        "scratch one float short": call(floats=need - 1),
        "scratch 0": call(floats=0),
    }
    return (keep, hraw), cases


def test_window_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    keep, cases = _window_cases()
    for what, args in cases.items():
        lib.narde_version()
        rc = lib.narde_value_td_window(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
    # the messages name what is wrong
    for what, word in (("lam 1.5", b"lam"), ("plies 0", b"plies"), ("records misaligned", b"records"),
                       ("scratch misaligned", b"scratch"), ("scratch one float short", b"NARDE_TD_WINDOW_SCRATCH_FLOATS"),
                       ("ld_w1 < 198", b"ld_w1")):
        assert lib.narde_value_td_window(*cases[what]) == -1 and word in lib.narde_last_error(), what
    del keep


def test_records_rollouts_refuse_a_misaligned_records_and_keep_the_parents_errors():
    lib = _lib.load()
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    hraw, h = _handle()
    net = _lib.ValueMlp(buf, 80, buf, buf, buf, 80, 0, 2)
    R, N = ctypes.byref, None

    def ref2(handle=h, plies=3, w=R(net), eps=N, tag=N, actions=buf, records=buf):
        return (handle, plies, w, w, eps, 7, tag, buf, actions, buf, buf, buf, buf, records, N)

    def full4(handle=h, plies=3, w=R(net), eps=N, tag=N, play=buf, scratch=buf, nbytes=_lib.turn_rollout_scratch_bytes(1),
              records=buf):
        return (handle, plies, w, w, eps, 7, tag, buf, play, buf, buf, buf, buf, scratch, nbytes, records, N)

    for name, call, column in (("narde_value_rollout_records", ref2, "actions"),
                               ("narde_turn_value_rollout_records", full4, "play")):
        fn = getattr(lib, name)
        cases = {"records misaligned": call(records=odd), "NULL handle": call(handle=N), "plies 0": call(plies=0),
                 "no net": call(w=N), "epsilon without tag": call(eps=buf),
                 f"{column} misaligned": call(**{column: ctypes.c_void_p(buf.value + 2)})}
        if call is full4:
            cases.update({"NULL scratch": call(scratch=N), "scratch misaligned": call(scratch=odd),
                          "scratch below one piece": call(nbytes=16)})
        for what, args in cases.items():
            lib.narde_version()
            assert fn(*args) == -1, f"{name}: {what}"
            assert lib.narde_last_error(), what
        assert fn(*call(records=odd)) == -1 and b"records" in lib.narde_last_error()
    del keep, hraw
