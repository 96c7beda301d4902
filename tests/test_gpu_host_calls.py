"""GPU: the narde_host_* calls (host arrays, n <= 4096: what the scalar facade
runs on) against the device entry points they wrap.

Each host call stages its arrays through the handle's pinned and device
buffers, one 256-byte-aligned slot per array, runs the same kernels on the
handle's private envs and copies the results back.  So for the same
positions, dice and actions it must return, bit for bit, what the device path
(narde_set_state, the call, narde_get_state on a fresh handle of n envs)
returns.  Sizes: 1 and 2 (consecutive arrays differ by the slot rounding
alone), kBlock + 1 (a second workgroup) and 4096 (the cap).  Refusals are
checked by return code and exact text; every one is refused on the host,
before any launch.  Positions, dice and actions: tests/golden/steps.npz."""
import numpy as np
import pytest
from conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K_BLOCK = 256    # device_common.h kBlock
HOST_CAP = 4096  # narde.hip kHostCap
SIZES = [1, 2, K_BLOCK + 1, HOST_CAP]
NOT_EXECUTABLE = ("move (%d, %d) at index %d is not executable: the source holds none of the "
                  "mover's checkers or the target holds opponent checkers")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def host():
    """One handle for every host call of the module (its own envs: 1)."""
    from gym_narde import _lib

    h = _lib.Handle(0, 1)
    yield h
    h.close()


@pytest.fixture(scope="module")
def steps():
    return golden("steps.npz")


_cases = {}


def case(steps, n):
    """n recorded steps (spread over the games, repeated if there are too few)
    and what the device path makes of them; computed once per n, read-only."""
    if n in _cases:
        return _cases[n]
    from gym_narde import _lib

    idx = (1000 + 7 * np.arange(n)) % len(steps["board"])
    c = {k: np.ascontiguousarray(steps[k][idx]) for k in
         ("board", "off", "first_turn", "player", "dice", "action", "list1", "count1")}
    # get_valid_moves' roll: two dice, a double as four
    c["dice4"] = np.zeros((n, 4), np.uint8)
    c["dice4"][:, :2] = c["dice"]
    dbl = c["dice"][:, 0] == c["dice"][:, 1]
    c["dice4"][dbl] = c["dice"][dbl, :1]
    # one listed move per env (from < 0: none listed, the env is skipped)
    c["move"] = np.where((c["count1"] > 0)[:, None], c["list1"][:, 0], -1).astype(np.int8)
    assert (c["move"][:, 0] >= 0).any() or n <= 2

    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    P = _lib.ptr
    h = _lib.Handle(0, n, max_episode_steps=0)  # the host calls step without a TimeLimit
    pos = [up(c[k]) for k in ("board", "off", "first_turn", "player")]

    def set_state():
        h.call("narde_set_state", *(P(t) for t in pos), None, None)

    def get_state():
        st = [new((n, 24), torch.int8), new((n, 2), torch.uint8), new((n, 2), torch.uint8), new((n,), torch.int8)]
        h.call("narde_get_state", *(P(t) for t in st), None, None)
        return st

    ref = {}
    # narde_step, given dice and actions, no auto-reset
    set_state()
    act, dice = up(c["action"]), up(c["dice"])
    obs, rew, term = new((n, 24), torch.int32), new((n,), torch.int32), new((n,), torch.uint8)
    h.call("narde_step", P(act), P(dice), P(obs), P(rew), P(term), None, None, None, 0, None)
    ref["step"] = get_state() + [obs, rew, term]
    # narde_legal_moves
    set_state()
    d4 = up(c["dice4"])
    count, moves = new((n,), torch.int16), new((n, _lib.MAX_MOVES, 2), torch.int8)
    h.call("narde_legal_moves", P(d4), P(count), P(moves), None, None)
    ref["legal"] = [count, moves]
    # narde_apply_moves
    set_state()
    mv = up(c["move"])
    h.call("narde_apply_moves", P(mv), P(pos[3]), None)
    ref["apply"] = get_state()[:3]
    # narde_violates_block_rule
    out = new((n,), torch.uint8)
    _lib.check(h.lib.narde_violates_block_rule(0, P(pos[0]), n, P(out), None), "narde_violates_block_rule")
    ref["block"] = [out]
    torch.cuda.synchronize()
    c["ref"] = {k: [t.cpu().numpy() for t in v] for k, v in ref.items()}
    h.close()
    for a in list(c.values()) + [a for v in c["ref"].values() for a in v]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _cases[n] = c
    return c


def position(c):
    """Writable copies of the case's position block."""
    return [c[k].copy() for k in ("board", "off", "first_turn", "player")]


def host_step(host, n, c, outputs=True):
    from gym_narde._lib import ptr

    st = position(c)
    out = [np.full((n, 24), -99, np.int32), np.full(n, -99, np.int32), np.full(n, 99, np.uint8)] if outputs else []
    host.call("narde_host_step", n, *(ptr(a) for a in st), ptr(c["dice"]), ptr(c["action"]),
              *(ptr(a) for a in out or [None] * 3))
    return st + out


def host_legal(host, n, c, with_moves=True):
    from gym_narde import _lib

    count = np.full(n, -99, np.int16)
    moves = np.full((n, _lib.MAX_MOVES, 2), 99, np.int8) if with_moves else None
    host.call("narde_host_legal_moves", n, *(_lib.ptr(c[k]) for k in ("board", "off", "first_turn", "player")),
              _lib.ptr(c["dice4"]), _lib.ptr(count), _lib.ptr(moves))
    return [count, moves] if with_moves else [count]


def same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert np.array_equal(g, w), (what, k, np.nonzero((g != w).reshape(len(g), -1).any(1))[0][:8])


@pytest.mark.parametrize("n", SIZES)
def test_host_step_equals_device_step(host, steps, n):
    c = case(steps, n)
    same(host_step(host, n, c), c["ref"]["step"], "step")
    # the three optional outputs NULL: the position alone
    same(host_step(host, n, c, outputs=False), c["ref"]["step"][:4], "step, no outputs")
    if n == HOST_CAP:  # the sample is no fixed point of the step
        assert (c["ref"]["step"][0] != c["board"]).any()


@pytest.mark.parametrize("n", SIZES)
def test_host_legal_moves_equals_device(host, steps, n):
    c = case(steps, n)
    same(host_legal(host, n, c), c["ref"]["legal"], "legal")
    same(host_legal(host, n, c, with_moves=False), c["ref"]["legal"][:1], "legal, counts only")
    if n == HOST_CAP:
        assert (c["ref"]["legal"][0] > 1).any() and (c["dice4"][:, 3] > 0).any()


@pytest.mark.parametrize("n", SIZES)
def test_host_apply_moves_equals_device(host, steps, n):
    from gym_narde._lib import ptr

    c = case(steps, n)
    st = position(c)
    host.call("narde_host_apply_moves", n, *(ptr(a) for a in st), ptr(c["move"]))
    same(st[:3], c["ref"]["apply"], "apply")
    assert np.array_equal(st[3], c["player"])  # an input
    if n == HOST_CAP:
        assert (c["ref"]["apply"][0] != c["board"]).any()


@pytest.mark.parametrize("n", SIZES)
def test_host_block_rule_equals_device(host, steps, n):
    from gym_narde._lib import ptr

    c = case(steps, n)
    out = np.full(n, 99, np.uint8)
    host.call("narde_host_violates_block_rule", n, ptr(c["board"]), ptr(out))
    same([out], c["ref"]["block"], "block")


def refused(host, name, *args):
    """The call's return code and error text."""
    rc = getattr(host.lib, name)(host.h, *args)
    return rc, host.lib.narde_last_error().decode()


def all_calls(c, n):
    """(name, arguments after the handle) of the four calls on the case's arrays."""
    from gym_narde._lib import ptr

    pos = [ptr(c[k]) for k in ("board", "off", "first_turn", "player")]
    return [("narde_host_legal_moves", (n, *pos, ptr(c["dice4"]), ptr(np.zeros(max(n, 1), np.int16)), None)),
            ("narde_host_step", (n, *pos, ptr(c["dice"]), ptr(c["action"]), None, None, None)),
            ("narde_host_apply_moves", (n, *pos, ptr(c["move"]))),
            ("narde_host_violates_block_rule", (n, pos[0], ptr(np.zeros(max(n, 1), np.uint8))))]


def test_batch_size_refusals_and_empty_batch(host, steps):
    c = case(steps, 2)
    for name, args in all_calls(c, 2):
        nulls = (None,) * (len(args) - 1)
        # the cap and the sign come before the pointers are looked at
        assert refused(host, name, HOST_CAP + 1, *nulls) == (-1, "host batch 4097 > 4096"), name
        assert refused(host, name, -1, *nulls) == (-1, "host batch -1 > 4096"), name
        # an empty batch is done, whatever the pointers
        assert getattr(host.lib, name)(host.h, 0, *nulls) == 0, name
        assert getattr(host.lib, name)(None, *args) == -1, name
        assert host.lib.narde_last_error() == b"NULL handle", name


def test_null_required_pointer_refused(host, steps):
    c = case(steps, 2)
    optional = {"narde_host_legal_moves": {7}, "narde_host_step": {7, 8, 9}}
    for name, args in all_calls(c, 2):
        for k in range(1, len(args)):
            if k in optional.get(name, ()):
                continue
            a = list(args)
            a[k] = None
            assert refused(host, name, *a) == (-1, "NULL argument"), (name, k)


def test_invalid_position_refused(host, steps):
    from gym_narde._lib import ptr

    c = dict(case(steps, 2))
    board = c["board"].copy()
    assert board[1].clip(min=0).sum() + c["off"][1, 0] == 15
    board[1, np.nonzero(board[1] == 0)[0][0]] = 1  # a sixteenth white checker, on an empty point
    c["board"] = board
    before = [a.copy() for a in position(c)]
    for name, args in all_calls(c, 2)[:3]:
        assert refused(host, name, *args) == (-1, "invalid position at index 1"), name
    assert all(np.array_equal(a, b) for a, b in zip(position(c), before))
    # the position is checked before the dice
    bad = c["dice"].copy()
    bad[0, 0] = 0
    pos = [ptr(c[k]) for k in ("board", "off", "first_turn", "player")]
    assert refused(host, "narde_host_step", 2, *pos, ptr(bad), ptr(c["action"]), None, None, None) == (
        -1, "invalid position at index 1")


@pytest.mark.parametrize("die,at", [(0, 0), (7, 3)])
def test_die_out_of_range_refused(host, steps, die, at):
    from gym_narde._lib import ptr

    c = case(steps, 2)
    dice = c["dice"].copy()
    dice.reshape(-1)[at] = die
    st = position(c)
    rc = refused(host, "narde_host_step", 2, *(ptr(a) for a in st), ptr(dice), ptr(c["action"]), None, None, None)
    assert rc == (-1, "die out of range at %d" % at)
    same(st, position(c), "refused step")


def test_non_executable_move_writes_nothing_back(host, steps):
    from gym_narde._lib import ptr
    from gym_narde.envs.narde import rotate_board

    n = K_BLOCK + 1
    c = case(steps, n)
    assert (c["move"][:, 0] >= 0).sum() > n // 2
    moves = c["move"].copy()
    i = n - 1  # the second workgroup's env
    # an empty point of the mover's perspective board as the source
    persp = c["board"][i] if c["player"][i] == 1 else rotate_board(c["board"][i])
    f = int(np.nonzero(persp == 0)[0][0])
    moves[i] = (f, 24)
    st = position(c)
    rc = refused(host, "narde_host_apply_moves", n, *(ptr(a) for a in st), ptr(moves))
    assert rc == (-1, NOT_EXECUTABLE % (f, 24, i))
    same(st, position(c), "refused apply")  # the other envs' executable moves included


def test_back_to_back_calls_on_one_handle(steps):
    """A step, then legal moves of another size, then a step again on a handle
    of their own: each call lays its arrays out from the start of the buffers."""
    from gym_narde import _lib

    h = _lib.Handle(0, 1)
    a, b = case(steps, K_BLOCK + 1), case(steps, 2)
    same(host_step(h, K_BLOCK + 1, a), a["ref"]["step"], "step")
    same(host_legal(h, 2, b), b["ref"]["legal"], "legal after step")
    same(host_legal(h, K_BLOCK + 1, a), a["ref"]["legal"], "legal, the step's size")
    same(host_step(h, 2, b), b["ref"]["step"], "step after legal")
    h.close()
