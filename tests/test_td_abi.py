"""narde_value_td_trace / narde_value_td_apply: exported, bound, and their
arguments validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes
import struct

from gym_narde import _lib


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("narde_value_td_trace", 8), ("narde_value_td_apply", 16)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    # narde_value_mlp_train: narde_value_mlp's 56 B, a pointer and an int64
    assert ctypes.sizeof(_lib.ValueMlpTrain) == 72
    assert _lib.ValueMlpTrain.w1.offset == 56 and _lib.ValueMlpTrain.ld_w1.offset == 64
    assert _lib.td_scratch_floats(1, 1) == 4 + 204
    assert _lib.td_scratch_floats(65, 80) == 68 + 2 * 16004


def _aligned(nbytes):
    """(keep-alive, a 16-B aligned address inside it)"""
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=2, w1=buf, ld_w1=198)
    f.update(kw)
    return _lib.ValueMlpTrain(**f)


def _cases():
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    # a stand-in for a handle: the checks read its env count (an int64 behind
    # the device index) for the scratch size and return before any launch
    hraw = ctypes.create_string_buffer(512)
    struct.pack_into("q", hraw, 8, 100)
    h = ctypes.cast(hraw, ctypes.c_void_p)
    R = ctypes.byref
    ok = _net(buf)
    P = 200 * 80 + 1
    ld = P + 3
    need = _lib.td_scratch_floats(100, 80)
    nets = {
        "NULL net": N,
        "NULL w1t": R(_net(buf, w1t=N)),
        "NULL b1": R(_net(buf, b1=N)),
        "NULL w2": R(_net(buf, w2=N)),
        "NULL b2": R(_net(buf, b2=N)),
        "hidden 0": R(_net(buf, hidden=0)),
        "hidden 129": R(_net(buf, hidden=129, ld_w1t=129)),
        "ld_w1t < hidden": R(_net(buf, ld_w1t=79)),
        "ld_w1 < 198": R(_net(buf, ld_w1=197)),
        "hidden_act 3": R(_net(buf, hidden_act=3)),
        "hidden_act -1": R(_net(buf, hidden_act=-1)),
        "out_act 3": R(_net(buf, out_act=3)),
        "out_act -1": R(_net(buf, out_act=-1)),
    }
    trace = {what: (h, n, 0.5, buf, ld, buf, buf, N) for what, n in nets.items()}
    trace.update({
        "NULL handle": (N, R(ok), 0.5, buf, ld, buf, buf, N),
        "NULL trace": (h, R(ok), 0.5, N, ld, buf, buf, N),
        "NULL v": (h, R(ok), 0.5, buf, ld, N, buf, N),
        "NULL black": (h, R(ok), 0.5, buf, ld, buf, N, N),
        "ld_trace < P": (h, R(ok), 0.5, buf, P - 1, buf, buf, N),
        "ld_trace not a multiple of 4": (h, R(ok), 0.5, buf, P + 1, buf, buf, N),
        "trace misaligned": (h, R(ok), 0.5, odd, ld, buf, buf, N),
    })

    def apply(handle=h, net=R(ok), trace=buf, ld_trace=ld, v=buf, black=buf, reward=buf, term=buf, trunc=buf,
              perspective=1, scratch=buf, floats=need, delta=N):
        return (handle, net, trace, ld_trace, v, black, reward, term, trunc, 0.1, 1.0, perspective, scratch, floats,
                delta, N)

    app = {what: apply(net=n) for what, n in nets.items()}
    app.update({
        "NULL handle": apply(handle=N),
        "NULL trace": apply(trace=N),
        "NULL v": apply(v=N),
        "NULL black": apply(black=N),
        "NULL reward": apply(reward=N),
        "NULL terminated": apply(term=N),
        "NULL truncated": apply(trunc=N),
        "NULL scratch": apply(scratch=N),
        "ld_trace < P": apply(ld_trace=P - 1),
        "ld_trace not a multiple of 4": apply(ld_trace=P + 2),
        "trace misaligned": apply(trace=odd),
        "perspective 0": apply(perspective=0),
        "perspective 2": apply(perspective=2),
        "scratch one float short": apply(floats=need - 1),
        "scratch 0": apply(floats=0),
        "scratch misaligned": apply(scratch=odd),
    })
    return (keep, hraw), trace, app


def test_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    keep, trace, app = _cases()
    for name, cases in (("narde_value_td_trace", trace), ("narde_value_td_apply", app)):
        for what, args in cases.items():
            lib.narde_version()
            rc = getattr(lib, name)(*args)
            assert rc == -1, f"{name}: {what} returned {rc}"
            msg = lib.narde_last_error()
            assert msg, what
    # the messages name what is wrong
    assert lib.narde_value_td_apply(*app["perspective 0"]) == -1 and b"perspective" in lib.narde_last_error()
    assert lib.narde_value_td_apply(*app["scratch one float short"]) == -1
    assert b"NARDE_TD_SCRATCH_FLOATS" in lib.narde_last_error()
    assert lib.narde_value_td_trace(*trace["ld_trace < P"]) == -1 and b"ld_trace" in lib.narde_last_error()
    del keep
