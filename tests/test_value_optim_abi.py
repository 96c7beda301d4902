"""narde_value_td_window_grad, narde_value_fit_grad, narde_value_grad_norm,
narde_value_sgd_step and narde_value_adam_step: exported, bound, and their
arguments validated before any device call (CPU-safe: no GPU is touched)."""
import ctypes

from gym_narde import _lib
from test_td_window_abi import B, _aligned, _handle, _net

N_SAMPLES = 300


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("narde_value_td_window_grad", 14), ("narde_value_fit_grad", 12), ("narde_value_grad_norm", 6),
                        ("narde_value_sgd_step", 6), ("narde_value_adam_step", 13)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    # the plain calls less alpha, with grad ahead of the stream
    a, b = _lib.SIGNATURES["narde_value_td_window"][1], _lib.SIGNATURES["narde_value_td_window_grad"][1]
    assert b == a[:7] + a[8:13] + [ctypes.c_void_p, ctypes.c_void_p]
    a, b = _lib.SIGNATURES["narde_value_fit"][1], _lib.SIGNATURES["narde_value_fit_grad"][1]
    assert b == a[:6] + a[7:11] + [ctypes.c_void_p, ctypes.c_void_p]


def _net_cases(buf, call):
    R, N = ctypes.byref, None
    return {
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
    }


def _check(fn, cases, words):
    lib = _lib.load()
    for what, args in cases.items():
        lib.narde_version()
        rc = fn(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
    for what, word in words:  # the messages name what is wrong
        assert fn(*cases[what]) == -1 and word in lib.narde_last_error(), what


def test_window_grad_argument_errors_are_einval_before_any_device_call():
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    hraw, h = _handle()
    ok = _net(buf)
    need = _lib.td_window_scratch_floats(B, 3, 80)

    def call(handle=h, net=ctypes.byref(ok), plies=3, records=buf, reward=buf, term=buf, trunc=buf, lam=0.7, scratch=buf,
             floats=need, delta=N, grad=buf):
        return (handle, net, plies, records, reward, term, trunc, lam, 1.0, scratch, floats, delta, grad, N)

    cases = _net_cases(buf, call)
    cases.update({
        "NULL handle": call(handle=N),
        "plies 0": call(plies=0, floats=10 ** 9),
        "plies past 2^31 samples": call(plies=2 ** 31 // B, floats=2 ** 62),
        "NULL records": call(records=N),
        "NULL reward": call(reward=N),
        "NULL terminated": call(term=N),
        "NULL truncated": call(trunc=N),
        "NULL scratch": call(scratch=N),
        "lam 1.5": call(lam=1.5),
        "lam NaN": call(lam=float("nan")),
        "records misaligned": call(records=odd),
        "scratch misaligned": call(scratch=odd),
        "scratch one float short": call(floats=need - 1),
        "NULL grad": call(grad=N),
        "grad misaligned": call(grad=odd),
    })
    _check(_lib.load().narde_value_td_window_grad, cases,
           (("grad misaligned", b"grad"), ("lam 1.5", b"lam"), ("scratch one float short", b"NARDE_TD_WINDOW_SCRATCH_FLOATS"),
            ("records misaligned", b"records")))
    del keep, hraw


def test_fit_grad_argument_errors_are_einval_before_any_device_call():
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    ok = _net(buf)
    need = _lib.value_fit_scratch_floats(N_SAMPLES, 80)

    def call(device=0, net=ctypes.byref(ok), n=N_SAMPLES, records=buf, target=buf, weight=N, scratch=buf, floats=need,
             v=N, loss=N, grad=buf):
        return (device, net, n, records, target, weight, scratch, floats, v, loss, grad, N)

    cases = _net_cases(buf, call)
    cases.update({
        "device -1": call(device=-1),
        "NULL records": call(records=N),
        "NULL target": call(target=N),
        "NULL scratch": call(scratch=N),
        "n 0": call(n=0),
        "n 2^31": call(n=2 ** 31, floats=2 ** 62),
        "records misaligned": call(records=odd),
        "scratch misaligned": call(scratch=odd),
        "scratch one float short": call(floats=need - 1),
        "loss misaligned": call(loss=odd),
        "NULL grad": call(grad=N),
        "grad misaligned": call(grad=odd),
    })
    _check(_lib.load().narde_value_fit_grad, cases,
           (("grad misaligned", b"grad"), ("n 0", b"n 0"), ("scratch one float short", b"NARDE_VALUE_FIT_SCRATCH_FLOATS"),
            ("loss misaligned", b"loss"), ("device -1", b"device")))
    del keep


def test_norm_argument_errors_are_einval_before_any_device_call():
    N = None
    keep, buf = _aligned(512)

    def call(device=0, hidden=80, grad=buf, max_norm=1.0, out=buf):
        return (device, hidden, grad, max_norm, out, N)

    cases = {
        "device -1": call(device=-1),
        "hidden 0": call(hidden=0),
        "hidden 129": call(hidden=129),
        "NULL grad": call(grad=N),
        "NULL out": call(out=N),
        "grad misaligned": call(grad=ctypes.c_void_p(buf.value + 4)),
        "out misaligned": call(out=ctypes.c_void_p(buf.value + 2)),
        "max_norm -1": call(max_norm=-1.0),
        "max_norm NaN": call(max_norm=float("nan")),
    }
    _check(_lib.load().narde_value_grad_norm, cases,
           (("hidden 129", b"hidden"), ("max_norm -1", b"max_norm"), ("grad misaligned", b"grad"), ("out misaligned", b"out")))
    del keep


def test_sgd_argument_errors_are_einval_before_any_device_call():
    N = None
    keep, buf = _aligned(512)
    ok = _net(buf)

    def call(device=0, net=ctypes.byref(ok), grad=buf, scale=N, alpha=0.1):
        return (device, net, grad, scale, alpha, N)

    cases = _net_cases(buf, call)
    cases.update({
        "device -1": call(device=-1),
        "NULL grad": call(grad=N),
        "grad misaligned": call(grad=ctypes.c_void_p(buf.value + 4)),
        "scale misaligned": call(scale=ctypes.c_void_p(buf.value + 2)),
        "alpha -1": call(alpha=-1.0),
        "alpha NaN": call(alpha=float("nan")),
    })
    _check(_lib.load().narde_value_sgd_step, cases,
           (("alpha -1", b"alpha"), ("scale misaligned", b"scale"), ("grad misaligned", b"grad"), ("ld_w1 < 198", b"ld_w1")))
    del keep


def test_adam_argument_errors_are_einval_before_any_device_call():
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    ok = _net(buf)

    def call(device=0, net=ctypes.byref(ok), grad=buf, scale=N, m=buf, s=buf, state=buf, lr=1e-3, beta1=0.9,
             beta2=0.999, eps=1e-8, wd=0.0):
        return (device, net, grad, scale, m, s, state, lr, beta1, beta2, eps, wd, N)

    cases = _net_cases(buf, call)
    cases.update({
        "device -1": call(device=-1),
        "NULL grad": call(grad=N),
        "NULL m": call(m=N),
        "NULL s": call(s=N),
        "NULL state": call(state=N),
        "grad misaligned": call(grad=odd),
        "m misaligned": call(m=odd),
        "s misaligned": call(s=odd),
        "state misaligned": call(state=odd),
        "scale misaligned": call(scale=ctypes.c_void_p(buf.value + 2)),
        "beta1 1": call(beta1=1.0),
        "beta1 -0.1": call(beta1=-0.1),
        "beta2 1": call(beta2=1.0),
        "beta2 NaN": call(beta2=float("nan")),
        "eps 0": call(eps=0.0),
        "eps -1": call(eps=-1.0),
        "lr -1": call(lr=-1.0),
        "lr NaN": call(lr=float("nan")),
        "weight_decay -1": call(wd=-1.0),
    })
    _check(_lib.load().narde_value_adam_step, cases,
           (("beta1 1", b"beta1"), ("eps 0", b"eps"), ("lr -1", b"lr"), ("weight_decay -1", b"weight_decay"),
            ("state misaligned", b"state"), ("m misaligned", b"m and s")))
    del keep
