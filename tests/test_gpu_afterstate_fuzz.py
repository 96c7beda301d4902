"""The afterstate, scoring, lookahead and TD kernels on positions random
self-play does not reach (tests/fuzz_positions.py: run-heavy boards where the
block rule decides, half of them on a double, and bear-off endgames with
stacks and checkers borne off on both sides).

What the positions are for:
  * a run-heavy board on a double has a level above the turn kernels' 256-node
    fast frontier: about one env in eight goes to the overflow list, against
    three of 1,003 in the self-play cases;
  * 291 such envs in one call are more than twice the overflow launches' 128
    one-wave workgroups, so a wave walks a second and a third env with the
    earlier env's keys still in its LDS frontier and its slab piece;
  * with the spread side replying, more than a hundred (row, roll) reply walks
    of one lookahead call are redone by k_turn_look_overflow, several rolls of
    one row and several rows of one wave's 64-word load among them;
  * the endgame half reads the feature encoding's branches for stacks above
    three checkers and for borne-off counts.

References: the enumerator over oracle.full4_turn (turn_afterstates_ref.py)
and the restatement over the oracle's primitives (test_afterstates_cpu.py),
bit for bit; torch float64 within 8 x E for every value, E the same
computation's float32-against-float64 difference on the same rows
(test_value_cpu.py, test_lookahead_cpu.py and test_td_cpu.py state the
argument); terminal rows exact.  Every reference is computed once per module.
Each case asserts on its reference what it was built to hold, before any
kernel runs.
"""
import numpy as np
import pytest

import turn_afterstates_ref as R
from fuzz_positions import spread_replier_states, turn_states
from test_afterstates_cpu import reference_afterstates
from test_value_cpu import make_net

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_lookahead as GL  # noqa: E402
import test_gpu_td as GTD  # noqa: E402
import test_gpu_turn_lookahead as GTL  # noqa: E402
from afterstate_checks import _check_pick, _env, _equal, np_  # noqa: E402
from test_gpu_value import SIGMOID80, check_values, expected, nets  # noqa: E402

KEYS = ("board", "off", "ft", "player", "dice")
RELU65 = (65, "relu", "tanh", 4)  # the odd H of test_gpu_value.py's list
FRONT = 256  # kTurnFront: the fast frontier's nodes a level
OVF_WAVES = 128  # kTurnOvfWaves: the overflow launches' one-wave workgroups


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tenv(st, **kw):
    return _env([st[k] for k in KEYS], rules="full4", **kw)


def _sub(st, idx):
    return {k: np.ascontiguousarray(np.asarray(st[k])[idx]) for k in KEYS}


def _halves_alternately(st):
    """The states of a fuzz_positions set, taken alternately from its run-heavy
    and its endgame half."""
    n = len(st["player"])
    return _sub(st, np.stack([np.arange(n // 2), n // 2 + np.arange(n // 2)], 1).reshape(-1))


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _sentinel_turn_rows(dev, B, rows, cap, feat=True):
    from gym_narde.vector import TurnAfterstates

    return TurnAfterstates(torch.zeros(B + 1, dtype=torch.int32, device=dev),
                           torch.full((rows,), -7, dtype=torch.int32, device=dev),
                           torch.full((rows, 4, 2), -7, dtype=torch.int8, device=dev),
                           torch.full((rows, 198), -7.0, dtype=torch.float32, device=dev) if feat else None,
                           torch.full((rows, 24), -7, dtype=torch.int32, device=dev) if feat else None,
                           torch.full((rows,), -7, dtype=torch.int8, device=dev), cap)


# ---------------------------------------------------------------- a, c: FULL4 rows and their values

@pytest.fixture(scope="module")
def turn_case():
    """256 states, 24,392 rows; 33 envs above 256 rows (up to 741)."""
    st = turn_states(256, 808)
    ref = R.enumerate_turns(*(st[k] for k in KEYS))
    cnt = np.diff(ref["offsets"])
    heavy = cnt > FRONT
    assert heavy.sum() >= 24 and (cnt == 0).any()
    assert (st["player"][heavy] == 1).any() and (st["player"][heavy] == -1).any()
    assert set(np.unique(ref["max_dice"])) >= {0, 1, 2, 3, 4}
    mover = st["player"][ref["row_env"]]
    assert all(((ref["reward"] == r) & (mover == c)).any() for r in (1, 2) for c in (1, -1))
    return st, ref


def test_full4_rows_equal_the_enumerator(turn_case):
    st, want = turn_case
    B = len(st["player"])
    env = _tenv(st)
    aft = env.turn_afterstates(dice=st["dice"], obs=True)
    total = int(want["offsets"][-1])
    assert aft.cap == total and aft.feat.shape == (total, 198)
    _equal(aft, want, action="play")
    lean = env.turn_afterstates(dice=st["dice"], feat=False)
    assert lean.feat is None and lean.obs is None
    for k in ("offsets", "row_env", "play", "reward"):
        assert np.array_equal(np_(getattr(lean, k)), want[k]), k
    count = env.turn_afterstates(dice=st["dice"], cap=0)
    assert count.cap == 0 and np.array_equal(np_(count.offsets), want["offsets"])
    # a cap inside an overflow env's rows, at an odd row
    o = want["offsets"]
    heavy = np.nonzero(np.diff(o) > FRONT)[0]
    e = int(heavy[len(heavy) // 2])
    cap = int(o[e]) + 128 + (int(o[e]) % 2 == 0)
    assert cap % 2 == 1 and o[e] < cap < o[e + 1] and cap < total
    out = _sentinel_turn_rows(env.device, B, total, cap)
    cut = env.turn_afterstates(dice=st["dice"], out=out)
    assert cut.cap == cap
    _equal(cut, want, rows=cap, action="play")  # offsets: the true counts
    for a in (cut.row_env, cut.play, cut.feat, cut.obs, cut.reward):
        assert (np_(a)[cap:] == -7).all()
    env.close()


@pytest.mark.parametrize("perspective", ["white", "mover"])
def test_full4_pick_and_step(turn_case, perspective):
    """pick_turn against torch's segment extrema, and the picked plays carried
    out by the step: the position, obs and reward are the picked rows'."""
    st, want = turn_case
    env = _tenv(st)
    aft = env.turn_afterstates(dice=st["dice"], obs=True)
    rng = np.random.default_rng(9)
    v = rng.integers(0, 4, aft.cap).astype(np.float32) / 4 - 0.5  # four levels: ties everywhere
    values = torch.from_numpy(v).to(env.device)
    rows = _check_pick(env, aft, values, st["player"] == -1, perspective, want["play"])
    assert (rows == -1).sum() == (np.diff(want["offsets"]) == 0).sum()
    play, row = env.pick_turn(aft, values, perspective=perspective)
    obs, reward, term, _, _ = env.step(play, st["dice"])
    feat = np_(env.tesauro198())
    s = env.get_state()
    has = rows >= 0
    r = rows[has].astype(np.int64)
    assert np.array_equal(np_(s["board"])[has], want["board"][r]) and np.array_equal(np_(s["off"])[has], want["off"][r])
    assert np.array_equal(np_(s["player"])[has], want["player"][r])
    assert np.array_equal(feat[has].view(np.uint32), want["feat"][r].view(np.uint32))
    assert np.array_equal(np_(obs)[has], want["obs"][r])
    assert np.array_equal(np_(reward)[has], want["reward"][r].astype(np.int32))
    assert np.array_equal(np_(term)[has] != 0, want["reward"][r] != 0)
    assert np.array_equal(np_(s["board"])[~has], st["board"][~has])  # no row: a pass
    env.close()


@pytest.mark.parametrize("spec", [SIGMOID80, RELU65], ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_full4_scored_values(turn_case, spec):
    st, want = turn_case
    env = _tenv(st)
    net, cpu = nets(spec, env.device)
    plain = env.turn_afterstates(dice=st["dice"])
    _equal(plain, want, action="play")
    for perspective in ("white", "mover"):
        aft, values = env.scored_turn_afterstates(net, dice=st["dice"], perspective=perspective)
        assert aft.feat is None and aft.cap == plain.cap
        for k in ("offsets", "row_env", "play", "reward"):
            assert torch.equal(getattr(aft, k), getattr(plain, k)), k
        exp, E, term = expected(cpu, plain.feat, plain.reward, perspective)
        assert term.any()
        check_values(values, exp, E, term, f"fuzz full4 {spec[:3]} {perspective}")
    env.close()


# ---------------------------------------------------------------- b: an overflow list longer than the grid

@pytest.fixture(scope="module")
def grid_case(turn_case):
    """491 envs: the first 48 states of turn_states(1024, 909) above 256 rows,
    six times over, 200 light states of turn_case between them, big_state()
    -- the slab tier -- first, in the middle and last.  The reference is
    computed once on the distinct states and tiled."""
    pool = turn_states(1024, 909)
    # above 256 rows: only a run-heavy board (the first half) on a double
    cand = np.nonzero(pool["dice"][:512, 0] == pool["dice"][:512, 1])[0][:112]
    lst, lref = turn_case
    lcnt = np.diff(lref["offsets"])
    light = np.sort(np.argsort(lcnt, kind="stable")[:200])  # the 200 with the fewest rows
    assert lcnt[light].max() <= 160 and np.median(lcnt[light]) < 32
    unit = R.concat(_sub(pool, cand), _sub(lst, light), R.big_states())
    uref = R.enumerate_turns(*(unit[k] for k in KEYS))
    heavy = np.nonzero(np.diff(uref["offsets"])[:len(cand)] > FRONT)[0][:48]
    assert len(heavy) == 48
    BIG = len(cand) + 200
    body = np.empty(488, np.int64)
    is_light = np.diff(np.arange(489) * 200 // 488) == 1
    body[is_light], body[~is_light] = len(cand) + np.arange(200), np.tile(heavy, 6)
    idx = np.concatenate([[BIG], body[:244], [BIG], body[244:], [BIG]])
    st = _sub(unit, idx)
    ou = uref["offsets"].astype(np.int64)
    cnt = np.diff(ou)[idx]
    offsets = np.zeros(len(idx) + 1, np.int32)
    offsets[1:] = np.cumsum(cnt)
    src = np.concatenate([np.arange(ou[u], ou[u + 1]) for u in idx])  # the tiled rows' rows of the unit reference
    ref = dict(offsets=offsets, row_env=np.repeat(np.arange(len(idx)), cnt).astype(np.int32), play=uref["play"][src],
               reward=uref["reward"][src])
    # more than two envs a wave of the overflow launches: some wave takes three
    assert (cnt > FRONT).sum() > 2 * OVF_WAVES and cnt[0] == cnt[245] == cnt[-1] == R.BIG_ROWS
    assert (cnt == 0).any() and (ref["reward"] != 0).any()
    return st, ref, uref, src


def _tiled_rows_equal(aft, ref, uref, src, dev):
    for k in ("offsets", "row_env", "play", "reward"):
        assert np.array_equal(np_(getattr(aft, k)), ref[k]), k
    s = torch.from_numpy(src).to(dev)
    if aft.feat is not None:
        assert torch.equal(aft.feat.view(torch.int32), torch.from_numpy(uref["feat"]).to(dev).view(torch.int32)[s])
    if aft.obs is not None:
        assert torch.equal(aft.obs, torch.from_numpy(uref["obs"]).to(dev)[s])


def test_overflow_list_longer_than_the_grid_rows(grid_case):
    st, ref, uref, src = grid_case
    env = _tenv(st)
    dev = env.device
    count = env.turn_afterstates(dice=st["dice"], cap=0)
    assert np.array_equal(np_(count.offsets), ref["offsets"])
    a = env.turn_afterstates(dice=st["dice"], obs=True)
    assert a.cap == len(src)
    _tiled_rows_equal(a, ref, uref, src, dev)
    # the list's order differs from call to call; the rows do not
    b = env.turn_afterstates(dice=st["dice"], obs=True)
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(_bits(x), _bits(y))
    env.close()


def test_overflow_list_longer_than_the_grid_scored(grid_case):
    st, ref, uref, src = grid_case
    env = _tenv(st)
    net, cpu = nets(SIGMOID80, env.device)
    aft, values = env.scored_turn_afterstates(net, dice=st["dice"])
    assert aft.feat is None and aft.cap == len(src)
    _tiled_rows_equal(aft, ref, uref, src, env.device)
    exp, E, term = expected(cpu, torch.from_numpy(uref["feat"]), torch.from_numpy(uref["reward"]), "white")
    check_values(values, exp[src], E, term[src], "fuzz full4 grid")
    again = env.scored_turn_afterstates(net, dice=st["dice"])[1]
    assert torch.equal(_bits(values), _bits(again))
    env.close()


def test_overflow_list_longer_than_the_grid_records(grid_case):
    """The record fill (k_turn_fill_rec, k_turn_overflow_rec) through the
    lookahead: the rows bit for bit, terminal rows' outcomes exact, the same
    bits on a second call.  NODOUBLES keeps the lookahead's own work down; its
    values have their own tests."""
    st, ref, uref, src = grid_case
    env = _tenv(st, dice_mode="nodoubles")
    net, _ = nets(GTL.TANH17, env.device)
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    assert aft.feat is None and aft.cap == len(src)
    _tiled_rows_equal(aft, ref, uref, src, env.device)
    term = ref["reward"] != 0
    assert np.array_equal(np_(values)[term], GTL.terminal_outcomes(st, aft)[term])
    one = env.scored_turn_afterstates(net, dice=st["dice"])[1]
    assert torch.equal(values[torch.from_numpy(term)], one[torch.from_numpy(term)])
    assert bool(torch.isfinite(values).all()) and float((values - one).abs().max()) > 1e-3  # two plies, not one
    again = env.lookahead_turn_afterstates(net, dice=st["dice"])[1]
    assert torch.equal(_bits(values), _bits(again))
    env.close()


# ---------------------------------------------------------------- d: REF2

@pytest.fixture(scope="module")
def ref2_case():
    """512 states alternately from both halves, the dice two independent
    draws; the run-heavy half alone has no terminal row."""
    s = _halves_alternately(turn_states(512, 111, doubles=0.0))
    st = tuple(s[k] for k in KEYS)
    ref = reference_afterstates(*st)
    cnt = np.diff(ref["offsets"])
    mover = st[3][ref["row_env"]]
    assert (ref["reward"] == 1).any() and (ref["reward"] == 2).any()
    assert ((ref["reward"] != 0) & (mover == 1)).any() and ((ref["reward"] != 0) & (mover == -1)).any()
    assert cnt.max() > 64 and (cnt == 0).any() and (ref["inexpressible"] > 0).any()
    return st, ref


def test_ref2_rows_and_scored_values(ref2_case):
    st, want = ref2_case
    env = _env(st)
    net, cpu = nets(SIGMOID80, env.device)
    plain = env.afterstates(dice=st[4], obs=True)
    assert plain.cap == int(want["offsets"][-1])
    _equal(plain, want)
    for perspective in ("white", "mover"):
        aft, values = env.scored_afterstates(net, dice=st[4], perspective=perspective)
        for k in ("offsets", "row_env", "codes", "reward"):
            assert torch.equal(getattr(aft, k), getattr(plain, k)), k
        exp, E, term = expected(cpu, plain.feat, plain.reward, perspective)
        check_values(values, exp, E, term, f"fuzz ref2 {perspective}")
    env.close()


def test_ref2_lookahead(ref2_case):
    st = tuple(np.ascontiguousarray(a[:128]) for a in ref2_case[0])
    env = _env(st)
    net, cpu = nets(SIGMOID80, env.device)
    one, v1 = env.scored_afterstates(net, dice=st[4])
    aft, values = env.lookahead_afterstates(net, dice=st[4])
    for k in ("offsets", "row_env", "codes", "reward"):
        assert torch.equal(getattr(aft, k), getattr(one, k)), k
    assert np.array_equal(np_(aft.offsets), ref2_case[1]["offsets"][:129])
    want, E, live = GL.expected(cpu, st, aft)
    assert (~live).any()
    GL.check(values, want, E, live, "fuzz ref2 lookahead")
    assert np.array_equal(np_(values)[~live], GL.terminal_outcomes(st, aft)[~live])
    env.close()


# ---------------------------------------------------------------- e: the FULL4 lookahead's redone walks

def test_full4_lookahead_with_many_redone_walks():
    """spread_replier_states(32, 707), the halves taken alternately so that the
    rows with redone walks lie across the whole row range: 333 rows, 117
    (row, roll) pairs above 256 reply rows on 43 rows, 33 of them with two or
    more, rows 62 and 190 among those -- one wave's, in one load."""
    st = _halves_alternately(spread_replier_states(32, 707))
    env = _tenv(st)
    net, cpu = nets(SIGMOID80, env.device)
    one, v1 = env.scored_turn_afterstates(net, dice=st["dice"])
    aft, values = env.lookahead_turn_afterstates(net, dice=st["dice"])
    GTL.same_rows(aft, one)
    total = aft.cap
    assert 256 < total <= GTL.SPLIT_ROWS
    c = GTL.row_replies("spread_repliers", st, aft)
    live = c["live"]
    cnt = np.stack([np.diff(r["offsets"]) for r in c["replies"]], 1)
    big = cnt > FRONT
    rows = np.nonzero(live)[0]
    twice = rows[big.sum(1) >= 2]
    print(f"rows {total}, reply rows {int(cnt.sum())}, pairs above {FRONT} reply rows {int(big.sum())} on "
          f"{int(big.any(1).sum())} rows, {len(twice)} rows with two or more")
    assert big.sum() >= 100 and len(twice) >= 10
    assert len(np.unique(twice % OVF_WAVES)) < len(twice)  # two of them are one overflow wave's
    want, E = GTL.expected(cpu, c)
    GTL.check(values, want, E, live, "fuzz full4 lookahead")
    assert np.array_equal(np_(values)[~live], GTL.terminal_outcomes(st, aft)[~live])
    GTL.check(GTL.composed(net, cpu, c), want, E, np.ones(int(live.sum()), bool), "fuzz full4 lookahead composed")
    assert float((values - v1).abs().max()) > 1e3 * GTL.TOL_FACTOR * E
    # a wave a row (cap above 3,072) gives the four-waves-a-row launch's bits
    cap = GTL.SPLIT_ROWS + 1
    out = _sentinel_turn_rows(env.device, len(st["player"]), cap, cap, feat=False)
    vals = torch.full((cap,), -7.0, dtype=torch.float32, device=env.device)
    wide, v = env.lookahead_turn_afterstates(net, dice=st["dice"], out=(out, vals))
    assert wide.cap == cap and torch.equal(wide.offsets, aft.offsets)
    assert torch.equal(_bits(v[:total]), _bits(values)) and (np_(vals)[total:] == -7).all()
    env.close()


# ---------------------------------------------------------------- f: the TD trace on stacks and borne-off checkers

@pytest.mark.parametrize("H,hact,oact", [(80, "sigmoid", "sigmoid"), (65, "relu", "tanh")], ids=lambda x: str(x))
def test_td_trace_and_apply_on_endgames(H, hact, oact):
    """One trace + step + apply on the 256 endgame states of turn_states(512,
    313): test_gpu_td.py's comparison and tolerance."""
    from gym_narde.vector import VecNardeEnv

    B = 256
    st = _sub(turn_states(2 * B, 313, doubles=0.0), np.arange(B, 2 * B))
    own = st["board"] * st["player"][:, None]
    assert ((own > 3).any(1)).sum() >= B // 4 and ((own < -3).any(1)).sum() >= B // 2  # stacks above three checkers
    assert (st["off"][:, 0] > 0).sum() >= B // 4 and (st["off"][:, 1] > 0).sum() >= B // 4
    assert ((st["off"] > 0).all(1)).sum() >= B // 4  # both sides have borne off
    env = VecNardeEnv(B, device="cuda:0", seed=5, autoreset=True, max_episode_steps=GTD.MAX_STEPS)
    env.set_state(st["board"], st["off"], st["ft"], st["player"], np.full(B, 3, np.int16))
    raw = GTD.Raw(make_net(H, hact, oact, seed=H), env.device, B)
    decay, alpha, gamma = 0.7, 0.05, 0.9
    p32, p64 = raw.params(torch.float32), raw.params(torch.float64)
    trace0 = raw.trace[:, :raw.P].cpu()
    raw.trace_call(env, decay)
    trace1 = raw.trace.clone()
    _, reward, term, trunc, _ = env.step(None, st["dice"])
    post = env.get_state()
    raw.apply_call(env, reward, term, trunc, alpha, gamma)
    torch.cuda.synchronize()
    reward, term, trunc = reward.cpu(), term.cpu(), trunc.cpu()
    black = torch.from_numpy((st["player"] == -1).astype(np.uint8))
    assert torch.equal(raw.black.cpu(), black)
    want = GTD.reference(p32, p64, (hact, oact), GTD.feat_of(st), GTD.feat_of(post), trace0, decay, reward, black, term,
                         trunc, alpha, gamma)
    what = f"fuzz td H={H} {hact}/{oact}"
    GTD.close(f"v {what}", raw.v, want["v"])
    GTD.close(f"trace {what}", trace1[:, :raw.P], want["trace"])
    GTD.close(f"delta {what}", raw.delta, want["delta"])
    GTD.close(f"theta {what}", raw.theta(), want["theta"])
    done = (term | trunc).bool()
    after = raw.trace[:, :raw.P].cpu()
    assert (after[done] == 0).all()
    assert torch.equal(after[~done].view(torch.int32), trace1[:, :raw.P].cpu()[~done].view(torch.int32))
    raw.padding_untouched()
    raw.mirror_is_exact()
    env.close()
