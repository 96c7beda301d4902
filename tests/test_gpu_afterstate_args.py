"""The host-side refusals and shortcuts of afterstate expansion and the
value-greedy pick (VecNardeEnv.afterstates / pick_afterstate, turn_afterstates
/ pick_turn), the same for both rule sets: every ValueError text, the (R,1)
values, and the cap = 0 pick that reads no row array.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 3
# per rule set: the expand and pick methods, the result tuple, the action
# field with its trailing shape and dtype, the pick's "no row" fill
KINDS = {
    "ref2": ("afterstates", "pick_afterstate", "Afterstates", "codes", (2,), torch.int16, 0),
    "full4": ("turn_afterstates", "pick_turn", "TurnAfterstates", "play", (4, 2), torch.int8, -1),
}
# the other rule set's methods that refuse by name (pick_afterstate has no guard)
OTHERS = {
    "ref2": (("turn_afterstates", ()), ("pick_turn", (None, None))),
    "full4": (("afterstates", ()),),
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(params=("ref2", "full4"))
def kind(request):
    import gym_narde.vector as V

    rules = request.param
    expand, pick, tup, field, shape, dt, fill = KINDS[rules]
    env = V.VecNardeEnv(B, device="cuda:0", seed=11, rules=rules)
    env.reset()  # the start position
    yield env, getattr(env, expand), getattr(env, pick), getattr(V, tup), field, shape, dt, fill, rules
    env.close()


def _refuses(text, fn, *a, **kw):
    with pytest.raises(ValueError) as err:
        fn(*a, **kw)
    assert text in str(err.value), str(err.value)


def test_expand_refusals(kind):
    env, expand, pick, tup, field, shape, dt, fill, rules = kind
    for name, args in OTHERS[rules]:
        _refuses(f'{name}() is rules="{"full4" if rules == "ref2" else "ref2"}" only', getattr(env, name), *args)
    _refuses("cap must be >= 0", expand, cap=-1)
    good = expand(obs=True)
    cap = good.cap
    assert cap >= B and getattr(good, field).shape == (cap,) + shape and getattr(good, field).dtype == dt
    _refuses("cap must be >= 0", expand, out=good, cap=-1)
    dev = env.device
    msg = lambda name, d: f"out.{name} must be a contiguous {d} device tensor of at least cap rows"  # noqa: E731
    # a wrong dtype
    _refuses(msg("offsets", torch.int32), expand, out=good._replace(offsets=good.offsets.to(torch.int64)))
    _refuses(msg(field, dt), expand, out=good._replace(**{field: getattr(good, field).to(torch.int32)}))
    _refuses(msg("feat", torch.float32), expand, out=good._replace(feat=good.feat.double()))
    _refuses(msg("reward", torch.int8), expand, out=good._replace(reward=good.reward.to(torch.int32)))
    # fewer rows than cap
    _refuses(msg("row_env", torch.int32), expand, out=good._replace(row_env=good.row_env[:cap - 1]))
    _refuses(msg("row_env", torch.int32), expand, out=good, cap=cap + 1)  # (the first array checked)
    _refuses(msg(field, dt), expand, out=good._replace(**{field: getattr(good, field)[:cap - 1]}))
    # not contiguous
    wide = torch.zeros((cap, 2 * 198), dtype=torch.float32, device=dev)
    _refuses(msg("feat", torch.float32), expand, out=good._replace(feat=wide[:, :198]))
    _refuses(msg("row_env", torch.int32), expand,
             out=good._replace(row_env=torch.zeros(2 * cap, dtype=torch.int32, device=dev)[::2]))
    # a wrong trailing shape
    _refuses(msg("offsets", torch.int32), expand,
             out=good._replace(offsets=torch.zeros(B + 2, dtype=torch.int32, device=dev)))
    _refuses(msg(field, dt), expand, out=good._replace(**{field: torch.zeros((cap, 8), dtype=dt, device=dev)}))
    _refuses(msg("obs", torch.int32), expand,
             out=good._replace(obs=torch.zeros((cap, 25), dtype=torch.int32, device=dev)))
    # on the CPU
    _refuses(msg("reward", torch.int8), expand, out=good._replace(reward=good.reward.cpu()))
    # and the untouched tuple is accepted, with the same rows
    again = expand(out=good._replace(offsets=torch.zeros_like(good.offsets)))
    assert again.cap == cap and int(again.offsets[B]) == cap


def test_pick_refusals_and_shortcuts(kind):
    env, expand, pick, tup, field, shape, dt, fill, rules = kind
    aft = expand()
    cap = aft.cap
    dev = env.device
    values = torch.linspace(-1, 1, cap, dtype=torch.float32, device=dev)
    msg = f"values must be float32, one per afterstate row (at least {cap}), on the env's device"
    _refuses(msg, pick, aft, values.double())
    _refuses(msg, pick, aft, values.cpu())
    _refuses(msg, pick, aft, values[:cap - 1])
    _refuses(msg, pick, aft, values.reshape(1, cap))
    _refuses("epsilon and tag go together", pick, aft, values, epsilon=0.5)
    _refuses("epsilon and tag go together", pick, aft, values, tag=3)
    _refuses("perspective must be one of ('mover', 'white')", pick, aft, values, perspective="black")
    # (R,1) values give the (R,) pick
    a1, r1 = pick(aft, values, perspective="mover")
    a2, r2 = pick(aft, values.reshape(cap, 1), perspective="mover")
    assert a1.shape == (B,) + shape and a1.dtype == dt and r1.dtype == torch.int32
    assert torch.equal(a1, a2) and torch.equal(r1, r2) and int(r1.min()) >= 0
    o = aft.offsets.cpu()
    assert torch.equal(r1.cpu(), o[1:] - 1)  # ascending values: each env's last row
    assert torch.equal(a1, getattr(aft, field)[r1.long()])
    # cap = 0: "no row" everywhere, and no row array is read
    none = expand(cap=0)
    assert none.cap == 0 and torch.equal(none.offsets, aft.offsets)
    bare = tup(none.offsets, None, None, None, None, None, 0)
    a0, r0 = pick(bare, torch.empty(0, dtype=torch.float32, device=dev))
    assert a0.shape == (B,) + shape and a0.dtype == dt
    assert (r0 == -1).all() and (a0 == fill).all()
