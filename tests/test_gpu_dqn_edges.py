"""The DQN learner's kernels (csrc/dqn_learner.hip) away from the one shape
the driver uses: batch sizes on both sides of every loop bound, duplicate ring
rows, the other side of every bookkeeping branch, ragged sampler batches, the
fused sampler's ring wrap, head codes off the table, and ragged ReLU widths.

Every comparison is either bit for bit against the same fp32 operations
written one torch op at a time (the kernels document their operation order),
or within a multiple of the reference's own rounding, E = max |torch fp32 -
torch fp64| on the same inputs (the rule of tests/test_value_cpu.py).  No
bound is taken from a kernel's output.  Every output that is shorter than its
buffer is followed by a sentinel tail that must survive the call."""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_dqn import _block_sum_order, _filled_replay, _uniforms  # noqa: E402

DEV = "cuda:0"
GAMMA = float(np.float32(0.99))  # exact in fp32: the fp64 references read the same number
SENT = -7.0                      # no weight, TD error, reward or observation is negative
TOL_FACTOR = 8                   # x E, the reference's own rounding
kLossCache, kLearnThreads = 4, 1024
CACHED = kLossCache * kLearnThreads  # rows k_dqn_loss_prio keeps in registers


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same_bits(a, b):
    """Equal shape, dtype and bit patterns (-0.0 != 0.0, a NaN equals itself)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = torch.int32 if a.element_size() == 4 else torch.int64
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def f32(x):
    return torch.full((), x, dtype=torch.float32, device=DEV)


# ------------------------------------------------------- k_dqn_loss_prio
def _loss_inputs(B, max_at, clamp_rows, seed=12):
    """The existing loss test's inputs at batch B, with the largest raw weight
    at row max_at and |t1 - q1| + |t2 - q2| > 100 on clamp_rows."""
    g = torch.Generator(device=DEV).manual_seed(seed + B)
    rnd = lambda: torch.randn(B, device=DEV, generator=g)  # noqa: E731
    q1, q2, m1, m2 = rnd(), rnd(), rnd(), rnd()
    r = (torch.rand(B, device=DEV, generator=g) < 0.1).float() * 2
    d = (torch.rand(B, device=DEV, generator=g) < 0.2).float()
    w_raw = torch.rand(B, device=DEV, generator=g) * 5 + 0.1
    w_raw[max_at] = 7.5
    if len(clamp_rows):
        rows = torch.tensor(clamp_rows, device=DEV)
        q1[rows] = 90.0
        q2[rows] = -70.0
    return SimpleNamespace(B=B, q1=q1, q2=q2, m1=m1, m2=m2, r=r, d=d, w_raw=w_raw)


def _clamp_rows(B, clamp_single):
    if B == 1:
        return [0] if clamp_single else []
    rows = {1 % B, B // 3, B // 2, B - 2}
    if B > CACHED:
        rows.add(B - 1)  # a row past the register cache
    return sorted(rows)


def _loss_reference(x):
    """k_dqn_loss_prio's documented fp32 operations, one torch op each, and
    torch's autograd of the reference loss in fp32 and fp64."""
    B = x.B
    w_n = x.w_raw / x.w_raw.max()
    nd = (1 - x.d) * GAMMA
    t1 = x.r + nd * x.m1
    t2 = x.r + nd * x.m2
    e1, e2 = x.q1 - t1, x.q2 - t2
    raw = (t1 - x.q1).abs() + (t2 - x.q2).abs()
    td = torch.clamp(raw, 0.0, 100.0)
    inv_b = f32(1.0) / f32(float(B))
    gw = inv_b * w_n
    g1 = gw * (2 * e1)
    g2 = gw * (2 * e2)
    # the kernel DIVIDES each sum by (float)B.  Both operands are device
    # tensors here: torch turns `tensor / python_number` on the GPU into a
    # multiplication by the reciprocal, one ulp off for a B that is no power
    # of two (measured: B = 1,000, 4,095, 5,000 differed in the last bit)
    bt = f32(float(B))
    loss = _block_sum_order(w_n * (e1 * e1)) / bt + _block_sum_order(w_n * (e2 * e2)) / bt

    def autograd(dtype):
        c = lambda v: v.to(dtype)  # noqa: E731
        w = c(x.w_raw) / c(x.w_raw).max()
        a1, a2 = c(x.q1).clone().requires_grad_(), c(x.q2).clone().requires_grad_()
        u1 = c(x.r) + (1 - c(x.d)) * GAMMA * c(x.m1)
        u2 = c(x.r) + (1 - c(x.d)) * GAMMA * c(x.m2)
        lo = (w * (a1 - u1) ** 2).mean() + (w * (a2 - u2) ** 2).mean()
        lo.backward()
        return lo.detach().double(), a1.grad.double(), a2.grad.double()

    l32, a32, b32 = autograd(torch.float32)
    l64, a64, b64 = autograd(torch.float64)
    return SimpleNamespace(w_n=w_n, raw=raw, td=td, g1=g1, g2=g2, loss=loss, loss64=l64, g1_64=a64, g2_64=b64,
                           E_loss=float((l32 - l64).abs()), E_g1=float((a32 - a64).abs().max()),
                           E_g2=float((b32 - b64).abs().max()))


def _call_loss(rp, x, idx, eps_val=0.5, eps_min=0.01, eps_decay=0.995, cursor_add=64, tag_val=7, with_copy=True,
               pad=96):
    """One narde_dqn_loss_prio call with w, td and idx the first B elements
    of longer buffers; returns the buffers and the device scalars."""
    B = x.B
    w_buf = torch.full((B + pad,), SENT, device=DEV)
    w_buf[:B] = x.w_raw
    td_buf = torch.full((B + pad,), SENT, device=DEV)
    idx_buf = torch.full((B + pad,), -1, dtype=torch.int64, device=DEV)
    idx_buf[:B] = idx
    eps = None if eps_val is None else f32(eps_val)
    tag = None if tag_val is None else torch.full((), tag_val, dtype=torch.int64, device=DEV)
    loss = f32(SENT)
    loss_copy = f32(SENT) if with_copy else None
    g1, g2 = rp.loss_prio_fused(x.q1, x.q2, x.m1, x.m2, x.r, x.d, w_buf[:B], GAMMA, td_buf[:B], loss, idx_buf[:B], eps,
                                eps_min, eps_decay, cursor_add=cursor_add, tag=tag, loss_copy=loss_copy)
    torch.cuda.synchronize()
    return SimpleNamespace(w_buf=w_buf, td_buf=td_buf, idx_buf=idx_buf, eps=eps, tag=tag, loss=loss,
                           loss_copy=loss_copy, g1=g1, g2=g2, pad=pad)


def _check_loss_values(x, ref, out, idx, label):
    """Everything k_dqn_loss_prio computes from the rows alone (not idx)."""
    B = x.B
    assert same_bits(out.w_buf[:B], ref.w_n), "w"
    assert same_bits(out.td_buf[:B], ref.td), "td"
    assert same_bits(out.g1, ref.g1) and same_bits(out.g2, ref.g2), "g"
    assert same_bits(out.loss, ref.loss), (float(out.loss), float(ref.loss))
    if out.loss_copy is not None:
        assert same_bits(out.loss_copy, out.loss)
    # sentinel tails: nothing at or past B is written (idx is read only)
    assert bool((out.w_buf[B:] == SENT).all()) and bool((out.td_buf[B:] == SENT).all())
    assert bool((out.idx_buf[B:] == -1).all()) and torch.equal(out.idx_buf[:B], idx)
    # against fp64 autograd, in units of torch fp32 autograd's own error
    err1 = float((out.g1.double() - ref.g1_64).abs().max())
    err2 = float((out.g2.double() - ref.g2_64).abs().max())
    errl = float((out.loss.double() - ref.loss64).abs())
    print(f"loss_prio {label}: E_g1 {ref.E_g1:.3e} err {err1:.3e} | E_g2 {ref.E_g2:.3e} err {err2:.3e} | "
          f"E_loss {ref.E_loss:.3e} err {errl:.3e} (loss {float(ref.loss64):.9g})")
    assert err1 <= TOL_FACTOR * ref.E_g1 and err2 <= TOL_FACTOR * ref.E_g2
    assert errl <= TOL_FACTOR * ref.E_loss


def _check_clamped(out, rp, clamp_rows):
    """The clamped rows' TD error is exactly 100.0, their priority 100 + eps."""
    rows = torch.tensor(clamp_rows, dtype=torch.int64, device=DEV)
    hundred = torch.full((len(clamp_rows),), 100.0, device=DEV)
    assert same_bits(out.td_buf[rows], hundred)
    assert same_bits(rp.prio[out.idx_buf[rows]], hundred + rp.epsilon)


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("B", [1, 37, 1000, 1024, 4095, 4097, 5000, 9000])
def test_loss_prio_batch_sizes(B, where):
    """k_dqn_loss_prio where its loops change shape: threads that hold no row
    (B <= 1,024), a register cache one row short (4,095), one uncached pass
    (4,097, 5,000) and three for some threads, two for others (9,000).  The
    largest raw weight sits at row B - 1 (uncached for B > 4,096) or row 0;
    some rows' TD error is clamped at 100 (for B = 1 the one row is clamped
    in the "last" case, not in the "first").  w, td, g1, g2 and the loss are
    bit for bit the documented fp32 operations (the loss's division by B
    with both operands on the device: see _loss_reference); g and the loss
    are also within 8 E of fp64 autograd (measured: docs/MEASUREMENT_LOG.md
    M.31); priorities, the untouched ring rows, the running
    max, epsilon, cursor, tag, counter and beta are exact."""
    cap = 20000
    rp = _filled_replay(n=cap, stride=64)
    max_at = B - 1 if where == "last" else 0
    clamp_rows = _clamp_rows(B, clamp_single=where == "last")
    x = _loss_inputs(B, max_at, clamp_rows)
    g = torch.Generator(device=DEV).manual_seed(100 + B)
    idx = torch.randperm(cap - 64, device=DEV, generator=g)[:B]
    ref = _loss_reference(x)
    # the inputs have the shape that reaches the paths
    assert int(x.w_raw.argmax()) == max_at and int((x.w_raw == x.w_raw.max()).sum()) == 1
    if B > CACHED and where == "last":
        assert max_at >= CACHED and float(x.w_raw[:CACHED].max()) < float(x.w_raw[max_at])
    over, under = ref.raw > 100.0, ref.raw < 100.0
    assert int(over.sum()) == len(clamp_rows) and bool(over[clamp_rows].all())
    if B > 1:
        assert len(clamp_rows) >= 3 and int(under.sum()) > 0
        assert (B <= CACHED) or int(over[CACHED:].sum()) > 0
    rp.pos_t.fill_(cap - 10)  # the cursor wraps
    snap = rp.prio.clone()
    maxp0, ctr0, beta0 = rp.max_prio.clone(), int(rp.sample_ctr), float(rp.beta_t)
    out = _call_loss(rp, x, idx)
    _check_loss_values(x, ref, out, idx, f"B={B} max@{where}")
    if clamp_rows:
        _check_clamped(out, rp, clamp_rows)
    pr = ref.td + rp.epsilon
    assert same_bits(rp.prio[idx], pr)
    rest = torch.ones(cap, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert int(rest.sum()) == cap - B and same_bits(rp.prio[rest], snap[rest])
    assert same_bits(rp.max_prio, torch.maximum(maxp0, pr.max()))
    half = f32(0.5)
    assert same_bits(out.eps, torch.where(half > 0.01, half * 0.995, half))
    assert int(rp.pos_t) == (cap - 10 + 64) % cap
    assert int(out.tag) == 8 and int(rp.sample_ctr) == ctr0 + 1
    assert float(rp.beta_t) == min(1.0, beta0 + rp.beta_increment)


def test_loss_prio_duplicate_rows():
    """PER samples with replacement: B = 5,000 samples over 300 ring rows, one
    row named 600 times on both sides of the register cache (j < 4,096 and
    j >= 4,096).  Each named row ends with the priority of ONE of its own
    samples, every other row is untouched, the running max is exact, and the
    values that do not depend on idx are exact as for distinct rows."""
    B, cap = 5000, 20000
    rp = _filled_replay(n=cap, stride=64)
    clamp_rows = _clamp_rows(B, True)
    x = _loss_inputs(B, B - 1, clamp_rows)
    ref = _loss_reference(x)
    g = torch.Generator(device=DEV).manual_seed(31)
    rows300 = torch.randperm(cap - 64, device=DEV, generator=g)[:300]
    idx = rows300[torch.randint(0, 300, (B,), device=DEV, generator=g)]
    hot = rows300[17]
    lo = torch.randperm(CACHED, device=DEV, generator=g)[:300]
    hi = CACHED + torch.randperm(B - CACHED, device=DEV, generator=g)[:300]
    idx[lo] = hot
    idx[hi] = hot
    is_hot = idx == hot
    assert int(is_hot[:CACHED].sum()) >= 300 and int(is_hot[CACHED:].sum()) >= 300 and int(is_hot.sum()) >= 600
    named = torch.unique(idx)
    assert named.numel() <= 300 and named.numel() < B // 10
    snap = rp.prio.clone()
    maxp0 = rp.max_prio.clone()
    out = _call_loss(rp, x, idx)
    _check_loss_values(x, ref, out, idx, "duplicates")
    pr = ref.td + rp.epsilon
    # prio[k] carries the bits of some sample j with idx_j == k
    match = rp.prio[idx].view(torch.int32) == pr.view(torch.int32)
    won = torch.zeros(cap, dtype=torch.bool, device=DEV)
    won[idx[match]] = True
    assert bool(won[named].all()) and int(won.sum()) == named.numel()
    rest = torch.ones(cap, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert int(rest.sum()) == cap - named.numel() and same_bits(rp.prio[rest], snap[rest])
    assert same_bits(rp.max_prio, torch.maximum(maxp0, pr.max()))


def test_loss_prio_other_bookkeeping_branches():
    """The side of each bookkeeping branch the driver's call never takes:
    epsilon at and below its floor, each optional scalar absent, a cursor
    that lands exactly on 0, beta reaching and staying at 1.0, a running max
    priority above every new priority; the sampling counter + 1 per call and
    the row values unchanged throughout."""
    B, cap = 1000, 20000
    rp = _filled_replay(n=cap, stride=64)
    x = _loss_inputs(B, B - 1, _clamp_rows(B, True))
    ref = _loss_reference(x)
    g = torch.Generator(device=DEV).manual_seed(7)
    idx = torch.randperm(cap - 64, device=DEV, generator=g)[:B]
    calls = 0
    ctr0 = int(rp.sample_ctr)

    def call(**kw):
        nonlocal calls
        out = _call_loss(rp, x, idx, **kw)
        calls += 1
        assert int(rp.sample_ctr) == ctr0 + calls
        assert same_bits(out.w_buf[:B], ref.w_n) and same_bits(out.td_buf[:B], ref.td)
        assert same_bits(out.g1, ref.g1) and same_bits(out.g2, ref.g2) and same_bits(out.loss, ref.loss)
        assert bool((out.w_buf[B:] == SENT).all()) and bool((out.td_buf[B:] == SENT).all())
        assert same_bits(rp.prio[idx], ref.td + rp.epsilon)
        return out

    # epsilon at / below the floor: unchanged, bit for bit
    for e in (0.01, 0.005):
        out = call(eps_val=e, eps_min=0.01)
        assert same_bits(out.eps, f32(e))
    # ... and one ulp above it: decayed (the comparison is strict, in fp32)
    above = torch.nextafter(f32(0.01), f32(1.0))
    out = call(eps_val=float(above), eps_min=0.01)
    assert same_bits(out.eps, above * 0.995)
    # epsilon absent, tag given
    out = call(eps_val=None, tag_val=41)
    assert out.eps is None and int(out.tag) == 42
    # tag absent, the cursor advanced
    rp.pos_t.fill_(500)
    out = call(tag_val=None, cursor_add=64)
    assert out.tag is None and int(rp.pos_t) == 564
    # cursor_add = 0: the cursor untouched (even a value the modulo would change)
    rp.pos_t.fill_(cap + 12345)
    out = call(cursor_add=0)
    assert int(rp.pos_t) == cap + 12345 and int(out.tag) == 8
    # no loss copy
    out = call(with_copy=False)
    assert out.loss_copy is None
    # a cursor that lands exactly on 0
    rp.pos_t.fill_(cap - 64)
    call(cursor_add=64)
    assert int(rp.pos_t) == 0
    # beta: half an increment below 1 gives exactly 1.0, and 1.0 stays
    one = torch.ones((), dtype=torch.float64, device=DEV)
    rp.beta_t.fill_(1.0 - rp.beta_increment / 2)
    assert float(rp.beta_t) < 1.0
    call()
    assert same_bits(rp.beta_t, one)
    call()
    assert same_bits(rp.beta_t, one)
    # a running max above every new priority keeps its bits
    big = f32(123456.789)
    rp.max_prio.copy_(big)
    assert float(big) > float((ref.td + rp.epsilon).max())
    call()
    assert same_bits(rp.max_prio, big)
    assert calls == 11


# ----------------------------------------------------------- the sampler
S_N, S_SS, S_STRIDE, S_LONG = 6000, 198, 1234, 4100
S_SEED, S_CTR, S_BETA, S_BETA_INC = 0x9E3779B97F4A, 5, 0.4, 0.001


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scalars():
    return (torch.full((), S_CTR, dtype=torch.int64, device=DEV),
            torch.full((), S_BETA, dtype=torch.float64, device=DEV))


def _per_sample(p, cdf, b, pad=40):
    from gym_narde import _lib

    P = _lib.ptr
    idx = torch.full((b + pad,), -1, dtype=torch.int64, device=DEV)
    w = torch.full((b + pad,), SENT, device=DEV)
    u = torch.full((b + pad,), SENT, device=DEV)
    ctr, beta = _scalars()
    scratch = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().narde_per_sample(0, P(p), P(cdf), p.numel(), b, S_SEED, P(ctr), P(beta), S_BETA_INC,
                                            P(idx), P(w), P(u), P(scratch), _stream()), "narde_per_sample")
    torch.cuda.synchronize()
    assert int(scratch.abs().sum()) == 0
    return SimpleNamespace(idx=idx, w=w, u=u, ctr=ctr, beta=beta, b=b)


def _per_sample_gather(rp, p, cdf, b, pad=40):
    from gym_narde import _lib

    P = _lib.ptr
    ss = rp.obs.shape[1]
    z = dict(device=DEV)
    idx = torch.full((b + pad,), -1, dtype=torch.int64, **z)
    w = torch.full((b + pad,), SENT, **z)
    s = torch.full((b + pad, ss), SENT, **z)
    ns = torch.full((b + pad, ss), SENT, **z)
    a = torch.full((b + pad, 2), -1, dtype=torch.int64, **z)
    r = torch.full((b + pad,), SENT, **z)
    d = torch.full((b + pad,), SENT, **z)
    ctr, beta = _scalars()
    _lib.check(_lib.load().narde_per_sample_gather(
        0, P(p), P(cdf), p.numel(), b, S_SEED, P(ctr), P(beta), P(idx), P(w), ss, P(rp.obs), rp.stride, rp.capacity,
        P(rp.action), P(rp.reward), P(rp.done), P(s), P(ns), P(a), P(r), P(d), _stream()), "narde_per_sample_gather")
    torch.cuda.synchronize()
    return SimpleNamespace(idx=idx, w=w, s=s, ns=ns, a=a, r=r, d=d, ctr=ctr, beta=beta, b=b)


@pytest.fixture(scope="module")
def sampler_case(need_gpu):
    """A 6,000-row ring with its pending rows at the end, its own prefix sums,
    one call of each sampler at batch 4,100 and that call's uniforms rebuilt
    on the host: computed once, read by every case below."""
    rp = _filled_replay(n=S_N, ss=S_SS, stride=S_STRIDE)
    assert rp.rows == S_N
    p, cdf = rp.prefix(S_N)
    torch.cuda.synchronize()
    return SimpleNamespace(rp=rp, p=p, cdf=cdf, long=_per_sample(p, cdf, S_LONG),
                           long_g=_per_sample_gather(rp, p, cdf, S_LONG), u=_uniforms(S_SEED, S_CTR, S_LONG))


@pytest.mark.parametrize("b", [1, 2, 3, 5, 63, 1023, 1025, 4099, S_LONG])
def test_sampler_small_and_ragged_batches(sampler_case, b):
    """k_per_sample / k_per_finish / k_per_sample_gather at batches that are
    no multiple of the 4 waves of a block and smaller than k_per_finish's
    1,024 threads.  Sample j's draw is keyed by (counter, j) alone: a call at
    batch b gives the first b picks, uniforms and raw weights of the call at
    batch 4,100 bit for bit; narde_per_sample's weights are the raw ones
    divided by the max of the first b; every pick obeys the search's
    invariant on the kernel's own prefix sums for the host-rebuilt uniform and
    has p > 0; beta and the counter step once (narde_per_sample) or not at
    all (narde_per_sample_gather); nothing at or past b is written."""
    c = sampler_case
    rp, p, cdf = c.rp, c.p, c.cdf
    ps = _per_sample(p, cdf, b)
    pg = _per_sample_gather(rp, p, cdf, b)
    # draw invariance
    assert same_bits(ps.idx[:b], c.long.idx[:b]) and same_bits(ps.u[:b], c.long.u[:b])
    assert same_bits(pg.idx[:b], c.long_g.idx[:b]) and same_bits(pg.w[:b], c.long_g.w[:b])
    assert same_bits(pg.idx[:b], ps.idx[:b])
    # normalised weights
    assert same_bits(ps.w[:b], pg.w[:b] / pg.w[:b].max())
    assert float(ps.w[:b].max()) == 1.0
    # scalars
    assert int(ps.ctr) == S_CTR + 1 and float(ps.beta) == min(1.0, S_BETA + S_BETA_INC)
    assert int(pg.ctr) == S_CTR and float(pg.beta) == S_BETA
    # the search invariant, for the uniforms rebuilt on the host
    assert same_bits(ps.u[:b], c.u[:b])
    idx = ps.idx[:b]
    v = c.u[:b] * cdf[S_N - 1]
    assert bool(((cdf[idx] > v) | (idx == S_N - 1)).all())
    assert bool(((idx == 0) | (cdf[(idx - 1).clamp(min=0)] <= v)).all())
    assert bool((p[idx] > 0).all()) and bool((rp.prio[idx] > 0).all())
    # the minibatch rows
    for got, src in ((pg.s, rp.obs[idx]), (pg.ns, rp.obs[(idx + rp.stride) % rp.capacity]), (pg.a, rp.action[idx]),
                     (pg.r, rp.reward[idx]), (pg.d, rp.done[idx])):
        assert same_bits(got[:b], src)
    # tails
    for t in (ps.idx, pg.idx, pg.a):
        assert bool((t[b:] == -1).all())
    for t in (ps.w, ps.u, pg.w, pg.s, pg.ns, pg.r, pg.d):
        assert bool((t[b:] == SENT).all())


def test_fused_sampler_ring_wrap():
    """k_per_sample_gather's next-observation wrap (kn >= cap): a full ring
    whose pending run lies in the middle, so rows with idx + stride >=
    capacity carry about a quarter of the mass.  ns is row (idx + stride) %
    capacity, s / a / r / d are row idx, bit for bit; no pending row is
    picked."""
    from gym_narde.dqn import DeviceReplay

    cap, stride, B = 6000, 1234, 4096
    rp = DeviceReplay(capacity=cap, state_size=198, device=DEV, stride=stride)
    g = torch.Generator(device=DEV).manual_seed(77)
    rp.obs.copy_(torch.rand(rp.obs.shape, device=DEV, generator=g))
    rp.reward.copy_(torch.rand(cap, device=DEV, generator=g))
    rp.done.copy_((torch.rand(cap, device=DEV, generator=g) < 0.2).float())
    rp.action.copy_(torch.randint(0, 576, (cap, 2), device=DEV, generator=g))
    rp.prio.copy_(torch.rand(cap, device=DEV, generator=g) * 3 + 0.01)
    rp.prio[2000:2000 + stride] = 0.0
    rp.size = cap - stride
    assert rp.rows == cap
    idx, _, s, ns, a, r, d = rp.sample_gather_fused(B, seed=21)
    torch.cuda.synchronize()
    wrapped = idx + stride >= cap
    assert int(wrapped.sum()) >= 100 and int((~wrapped).sum()) >= 100
    assert same_bits(ns, rp.obs[(idx + stride) % cap])
    assert same_bits(ns[wrapped], rp.obs[idx[wrapped] + stride - cap])
    assert same_bits(s, rp.obs[idx]) and same_bits(a, rp.action[idx])
    assert same_bits(r, rp.reward[idx]) and same_bits(d, rp.done[idx])
    assert bool((rp.prio[idx] > 0).all())


# ------------------------------------------------------ the gathered heads
HEAD_OUTPUTS = ("q1", "q2", "gf", "gw1", "gb1", "gw2", "gb2")
# x E_ref per output: the next power of two at or above twice the largest
# ratio measured over the cases below (docs/MEASUREMENT_LOG.md M.31)
HEAD_FACTORS = {"q1": 1, "q2": 1, "gf": 2, "gw1": 2, "gb1": 8, "gw2": 2, "gb2": 64}
OOR_CODES = (-5, 576, 2 ** 31 - 1)


def _head_codes(case, n, g):
    if case == "out_of_range":
        skew = torch.randint(0, 40, (n, 2), device=DEV, generator=g)
        wide = torch.randint(0, 576, (n, 2), device=DEV, generator=g)
        a = torch.where(torch.rand((n, 2), device=DEV, generator=g) < 0.7, skew, wide).to(torch.int64)
        off = torch.rand((n, 2), device=DEV, generator=g) < 0.1
        which = torch.randint(0, 3, (n, 2), device=DEV, generator=g)
        bad = torch.tensor(OOR_CODES, dtype=torch.int64, device=DEV)[which]
        a = torch.where(off, bad, a)
        for col in (0, 1):
            for code in OOR_CODES:
                assert int((a[:, col] == code).sum()) > 0
        share = float(((a < 0) | (a > 575)).double().mean())
        assert 0.07 < share < 0.13
        return a
    a = torch.empty((n, 2), dtype=torch.int64, device=DEV)
    a[:, 0] = 7
    a[:, 1] = 570
    return a


@pytest.mark.parametrize("case,n", [("out_of_range", 1000), ("one_code", 4096), ("one_code", 4100)])
def test_gathered_heads_vs_fp64_dense(case, n):
    """GatheredHeads against the dense heads + gather under autograd in
    FLOAT64: codes outside 0..575 (-5, 576, 2^31 - 1, in both columns; the
    reference clamps them), and every row on one code per head -- the longest
    run of k_heads_grad_w's ballot loop, every ballot full -- at one pass
    (4,096 rows) and with a second pass whose only rows sit in wave 0's first
    chunk (4,100).  Upstream gradients have |up| >= 0.5 and every feature row
    max_c f >= 0.5, so a dropped or doubled row moves a gradient entry by at
    least 0.25.  Per output the bound is HEAD_FACTORS x E_ref, E_ref = max
    |dense torch fp32 - dense torch fp64| measured here, the factors set from
    the ratios measured in docs/MEASUREMENT_LOG.md M.31; the bound is
    asserted to stay below 0.025, a tenth of a dropped row's effect."""
    from gym_narde.dqn import DecomposedDQN, gathered_heads

    torch.manual_seed(5)
    model = DecomposedDQN(198).cuda()
    g = torch.Generator(device=DEV).manual_seed(9 + n)
    f0 = torch.relu(torch.randn((n, 256), device=DEV, generator=g))
    rows = torch.arange(n, device=DEV)
    f0[rows, torch.randint(0, 256, (n,), device=DEV, generator=g)] = torch.rand(n, device=DEV, generator=g) + 0.5
    a = _head_codes(case, n, g)

    def upstream():
        sign = (torch.rand(n, device=DEV, generator=g) < 0.5).float() * 2 - 1
        return sign * (torch.rand(n, device=DEV, generator=g) + 0.5)

    up1, up2 = upstream(), upstream()
    assert float(up1.abs().min()) >= 0.5 and float(up2.abs().min()) >= 0.5
    assert float(f0.max(1).values.min()) >= 0.5

    def run(m, gathered, dtype):
        f = f0.detach().clone().to(dtype).requires_grad_(True)
        if gathered:
            q1, q2 = gathered_heads(m, f, a)
        else:
            ac = a.clamp(0, 575)
            q1 = m.move1_head(f).gather(1, ac[:, :1]).squeeze(1)
            q2 = m.move2_from_features(f, ac[:, 0]).gather(1, ac[:, 1:]).squeeze(1)
        for prm in m.parameters():
            prm.grad = None
        ((q1 * up1.to(dtype)).sum() + (q2 * up2.to(dtype)).sum()).backward()
        outs = [q1.detach(), q2.detach(), f.grad, m.move1_head.weight.grad, m.move1_head.bias.grad,
                m.move2_head.weight.grad, m.move2_head.bias.grad]
        return {k: v.double().clone() for k, v in zip(HEAD_OUTPUTS, outs)}

    got = run(model, True, torch.float32)
    d32 = run(copy.deepcopy(model), False, torch.float32)
    d64 = run(copy.deepcopy(model).double(), False, torch.float64)
    torch.cuda.synchronize()
    failed = []
    for k in HEAD_OUTPUTS:
        assert got[k].shape == d64[k].shape
        e_ref = float((d32[k] - d64[k]).abs().max())
        err = float((got[k] - d64[k]).abs().max())
        print(f"heads {case} n={n} {k}: E_ref {e_ref:.3e} err {err:.3e} ratio {err / e_ref:.2f} "
              f"bound {HEAD_FACTORS[k] * e_ref:.3e}")
        assert e_ref > 0 and HEAD_FACTORS[k] * e_ref < 0.025
        if not err <= HEAD_FACTORS[k] * e_ref:
            failed.append(k)
    assert not failed
    if case == "one_code":  # the other codes' gradient rows are written, as zeros
        assert bool((got["gw1"][torch.arange(576, device=DEV) != 7] == 0).all())
        assert bool((got["gw2"][torch.arange(576, device=DEV) != 570] == 0).all())


# -------------------------------------------- ReLU backward + bias gradient
@pytest.mark.parametrize("n,cols", [(1, 1), (63, 63), (65, 65), (130, 200), (64, 4096), (200, 257)])
def test_relu_bias_grad_ragged_widths(n, cols):
    """narde_relu_bias_grad at widths that are no multiple of a block's 64
    columns (the col < cols guard false inside a block), fewer than 4 slices
    of 64 rows (k_bias_grad_sum's quarters, some empty) and the widest
    accepted layer.  h holds exact 0.0 and -0.0 entries beside positive and
    negative ones.  g equals gh * (h > 0) and is bit for bit the selection
    autograd's threshold_backward makes, h > 0 ? gh : +0.0 (the product
    gh * 0 would carry gh's sign into the zero); db is within 8 E of the
    fp64 column sums, E = max |torch fp32 sum - fp64 sum|, and bit-identical
    on a second call; g and db are views into longer buffers whose sentinel
    borders survive."""
    from gym_narde import _lib
    from gym_narde.dqn import relu_bias_grad_scratch

    g = torch.Generator(device=DEV).manual_seed(1000 * n + cols)
    gh = torch.randn((n, cols), device=DEV, generator=g)
    h = torch.randn((n, cols), device=DEV, generator=g)
    kind = torch.randint(0, 6, (n, cols), device=DEV, generator=g)
    h = torch.where(kind == 0, torch.zeros_like(h), h)
    h = torch.where(kind == 1, -torch.zeros_like(h), h)
    if n * cols == 1:  # one entry: each kind in turn
        variants = [torch.full((1, 1), v, device=DEV) for v in (0.75, 0.0, -0.0)]
    else:
        flat = h.view(-1)
        flat[0] = 0.0
        flat[-1] = -0.0
        flat[1] = 0.5
        variants = [h]
    hb = torch.cat([v.view(-1) for v in variants]).view(torch.int32)
    assert int((hb == 0).sum()) > 0 and int((hb == -2 ** 31).sum()) > 0 and int((hb > 0).sum()) > 0
    border = 67  # floats: the views start off any 16-byte boundary
    scratch = relu_bias_grad_scratch(n, cols, DEV)
    P = _lib.ptr
    for h in variants:
        _relu_bias_grad_case(_lib, P, gh, h, n, cols, scratch, border)


def _relu_bias_grad_case(_lib, P, gh, h, n, cols, scratch, border):
    def call():
        g_buf = torch.full((n * cols + 2 * border,), SENT, device=DEV)
        db_buf = torch.full((cols + 2 * border,), SENT, device=DEV)
        gv = g_buf[border:border + n * cols].view(n, cols)
        dbv = db_buf[border:border + cols]
        _lib.check(_lib.load().narde_relu_bias_grad(0, P(gh), P(h), n, cols, P(gv), P(dbv), P(scratch), _stream()),
                   "narde_relu_bias_grad")
        torch.cuda.synchronize()
        for buf, size in ((g_buf, n * cols), (db_buf, cols)):
            assert bool((buf[:border] == SENT).all()) and bool((buf[border + size:] == SENT).all())
        return gv.clone(), dbv.clone()

    gv, dbv = call()
    assert torch.equal(gv, gh * (h > 0))
    assert same_bits(gv, torch.where(h > 0, gh, torch.zeros_like(gh)))
    want = gv.double().sum(0)
    E = float((gv.sum(0).double() - want).abs().max())
    err = float((dbv.double() - want).abs().max())
    print(f"relu_bias_grad ({n}, {cols}): E {E:.3e} err {err:.3e}")
    assert err <= TOL_FACTOR * E
    gv2, dbv2 = call()
    assert same_bits(gv2, gv) and same_bits(dbv2, dbv)
