"""narde_value_fit and narde_playout_targets: exported, bound, their constants
stated alike, and their arguments validated before any device call (CPU-safe:
no GPU is touched)."""
import ctypes

from gym_narde import _lib

N_SAMPLES = 300


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("narde_value_fit", 12), ("narde_playout_targets", 9)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.VALUE_FIT_SLAB == 128 == _lib.TD_WINDOW_SLAB
    # by hand: ceil(n / 128) partial rows of 200 H + 4 floats, two doubles a slab
    assert _lib.value_fit_scratch_floats(1, 1) == 204 + 4
    assert _lib.value_fit_scratch_floats(300, 80) == 3 * (16004 + 4)
    assert _lib.value_fit_scratch_floats(128, 128) == 25604 + 4
    assert _lib.value_fit_scratch_floats(129, 128) == 2 * (25604 + 4)


def _aligned(nbytes):
    """(keep-alive, a 16-B aligned address inside it)"""
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)


def _net(buf, **kw):
    f = dict(w1t=buf, ld_w1t=80, b1=buf, w2=buf, b2=buf, hidden=80, hidden_act=0, out_act=2, w1=buf, ld_w1=198)
    f.update(kw)
    return _lib.ValueMlpTrain(**f)


def _fit_cases():
    N = None
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    R = ctypes.byref
    ok = _net(buf)
    need = _lib.value_fit_scratch_floats(N_SAMPLES, 80)

    def call(device=0, net=R(ok), n=N_SAMPLES, records=buf, target=buf, weight=N, scratch=buf, floats=need, v=N, loss=N):
        return (device, net, n, records, target, weight, 0.1, scratch, floats, v, loss, N)

    cases = {
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
        "device -1": call(device=-1),
        "NULL records": call(records=N),
        "NULL target": call(target=N),
        "NULL scratch": call(scratch=N),
        "n 0": call(n=0),
        "n -5": call(n=-5),
        "n 2^31": call(n=2 ** 31, floats=2 ** 62),
        "records misaligned": call(records=odd),
        "scratch misaligned": call(scratch=odd),
        "scratch one float short": call(floats=need - 1),
        "scratch 0": call(floats=0),
        "loss misaligned": call(loss=odd),
    }
    return keep, cases


def test_fit_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    keep, cases = _fit_cases()
    for what, args in cases.items():
        lib.narde_version()
        rc = lib.narde_value_fit(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
    # the messages name what is wrong
    for what, word in (("n 0", b"n 0"), ("records misaligned", b"records"), ("scratch misaligned", b"scratch"),
                       ("scratch one float short", b"NARDE_VALUE_FIT_SCRATCH_FLOATS"), ("ld_w1 < 198", b"ld_w1"),
                       ("loss misaligned", b"loss"), ("device -1", b"device")):
        assert lib.narde_value_fit(*cases[what]) == -1 and word in lib.narde_last_error(), what
    del keep


def test_targets_argument_errors_are_einval_before_any_device_call():
    lib = _lib.load()
    keep, buf = _aligned(512)
    odd = ctypes.c_void_p(buf.value + 4)
    N = None

    def call(device=0, n=100, trials=4, sums=buf, leaf=N, roots=N, target=buf, weight=buf):
        return (device, n, trials, sums, leaf, roots, target, weight, N)

    cases = {
        "NULL sums": call(sums=N),
        "NULL target": call(target=N),
        "NULL weight": call(weight=N),
        "device -1": call(device=-1),
        "n 0": call(n=0),
        "n 2^31": call(n=2 ** 31),
        "trials 0": call(trials=0),
        "n x trials 2^31": call(n=2 ** 20, trials=2 ** 11),
        "roots misaligned": call(roots=odd),
    }
    for what, args in cases.items():
        lib.narde_version()
        rc = lib.narde_playout_targets(*args)
        assert rc == -1, f"{what} returned {rc}"
        assert lib.narde_last_error(), what
    for what, word in (("trials 0", b"trials"), ("roots misaligned", b"roots"), ("n 0", b"n 0")):
        assert lib.narde_playout_targets(*cases[what]) == -1 and word in lib.narde_last_error(), what
    del keep
