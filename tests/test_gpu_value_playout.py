"""Monte-Carlo playouts on the GPU (k_value_playout / k_turn_value_playout
through VecNardeEnv.playout and state_records), against
the one-launch rollouts that existed before them.

The oracle of a playout of N roots x `trials` trials is a second env of
B = N * trials envs made with the playout's seed, env_id_offset = id_base and
max_episode_steps = 0, set_state()-ed to every root `trials` times over and
set to the roots' ply counter: one value_rollout() / turn_value_rollout() of
max_plies plies with reward, terminated and records.  Env q's first terminal
ply gives trial q's length and outcome (its reward, negated where the record
that ply found has black to move); an env with none is an unfinished trial of
max_plies plies, and the env's position after the launch is the position its
leaf is the value of.  The existing GPU tests check those rollouts against the
composed per-ply calls.  Every integer output must equal the oracle's bit for
bit.

leaf: against the net's CPU twin in torch float64 on O.tesauro198 of the
oracle's stop positions, within TOL_FACTOR x E of tests/test_value_cpu.py,
E = max |torch float32 - torch float64| on the same rows floored at one
float32 ulp of the largest value (the reference's own rounding, as
test_value_rollout_cpu.judge floors it).
"""
import copy

import numpy as np
import pytest

import oracle as O
from fuzz_positions import random_positions
from test_value_cpu import TOL_FACTOR, make_net
from test_value_playout_cpu import late_races
from test_value_rollout_cpu import endgames
from turn_afterstates_ref import BIG_ROWS, big_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20251021
H128 = (128, "sigmoid", "sigmoid", 2)
H1 = (1, "tanh", "none", 3)
H17 = (17, "tanh", "none", 6)
H80 = (80, "sigmoid", "sigmoid", 1)
RULES = ("ref2", "full4")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def np_(x):
    return x.detach().cpu().numpy()


def make_env(B, rules, seed=SEED, id_base=0, dice_mode="all36", max_steps=0):
    from gym_narde.vector import VecNardeEnv

    return VecNardeEnv(B, device="cuda:0", seed=seed, env_id_offset=id_base, max_episode_steps=max_steps,
                       dice_mode=dice_mode, rules=rules)


_NETS = {}


def twins(spec):
    """(the net on the GPU, its CPU twin); one pair a spec for the module"""
    if spec is None:
        return None, None
    if spec not in _NETS:
        cpu = make_net(*spec)
        _NETS[spec] = (copy.deepcopy(cpu).to("cuda:0"), cpu)
    return _NETS[spec]


def start_position():
    sp = O.SelfPlay(1)
    sp.reset(0)
    return (sp.board[:1].astype(np.int8), sp.off[:1].astype(np.uint8), sp.ft[:1].astype(np.uint8),
            np.array([1], np.int8))


def concat(*states):
    return tuple(np.ascontiguousarray(np.concatenate([s[k] for s in states])) for k in range(4))


def seven_roots():
    """the start position, two fuzz middle-game positions (the first with white
    and the first with black to move), the four endgames"""
    f = random_positions(60, 17)[:4]
    mid = [int(np.flatnonzero(f[3][:30] == colour)[0]) for colour in (1, -1)]
    return concat(start_position(), tuple(a[mid] for a in f), endgames())


def oracle_run(rules, state, t, trials, max_plies, gw, gb, seed=SEED, id_base=0, dice_mode="all36", stop_feat=False):
    """The playout's numbers by the existing rollout (the module docstring)."""
    N = len(state[3])
    B = N * trials
    env = make_env(B, rules, seed, id_base, dice_mode)
    env.set_state(*(torch.as_tensor(np.repeat(a, trials, axis=0)).to(env.device) for a in state))
    env.ply = t
    if rules == "full4":
        bufs = env.turn_value_rollout_buffers(max_plies, dice=False, play=False, value=False, records=True)
        env.turn_value_rollout(max_plies, gw, gb, bufs=bufs)
    else:
        bufs = env.value_rollout_buffers(max_plies, dice=False, actions=False, value=False, records=True)
        env.value_rollout(max_plies, gw, gb, bufs=bufs)
    reward, term, rec = np_(bufs["reward"]), np_(bufs["terminated"]) != 0, np_(bufs["records"])
    assert not np_(bufs["truncated"]).any()
    done = term.any(0)
    first = np.where(done, term.argmax(0), max_plies - 1)
    q = np.arange(B)
    black = (rec[first, q, 6] >> 10) & 1
    outcome = np.where(done, np.where(black == 1, -1, 1) * reward[first, q], 0)
    length = first + 1
    o = dict(done=done.reshape(N, trials), outcome=outcome.reshape(N, trials).astype(np.int8),
             length=length.reshape(N, trials).astype(np.int32), records0=rec[0])
    o["sums"] = np.stack([o["done"].sum(1), o["outcome"].astype(np.int64).sum(1),
                          (o["outcome"].astype(np.int64) ** 2).sum(1), o["length"].sum(1)], 1).astype(np.int32)
    if stop_feat:  # the positions the unfinished trials stopped at (a finished env's has been reset: not used)
        st = {k: np_(v) for k, v in env.get_state().items()}
        o["feat"] = O.tesauro198(st["board"], st["off"], st["player"]).reshape(N, trials, 198)
        o["stop_player"] = st["player"].reshape(N, trials)
    env.close()
    return o


def run_playout(rules, state, t, trials, max_plies, gw, gb, seed=SEED, id_base=0, dice_mode="all36", **kw):
    caller = make_env(3, rules, seed=99, id_base=7, dice_mode=dice_mode, max_steps=1000)
    roots = caller.state_records(*state, t=t)
    res = caller.playout(roots, trials, gw, gb, max_plies=max_plies, seed=seed, id_base=id_base, per_trial=True, **kw)
    out = dict(sums=np_(res.sums), outcome=np_(res.outcome), length=np_(res.length),
               leaf=None if res.leaf is None else np_(res.leaf), res=res, roots=np_(roots))
    caller.close()
    return out


def assert_integers_equal(got, want, what=""):
    assert np.array_equal(got["length"], want["length"]), f"{what}: length"
    assert np.array_equal(got["outcome"], want["outcome"]), f"{what}: outcome"
    assert np.array_equal(got["sums"], want["sums"]), f"{what}: sums"


def check_leaf(got, want, gw_cpu, gb_cpu, what=""):
    """NaN exactly where the oracle's trial finished; elsewhere within
    TOL_FACTOR x E of the mover's net (the other colour's if it has none) in
    float64."""
    leaf, done = got["leaf"], want["done"]
    assert np.array_equal(np.isnan(leaf), done), f"{what}: leaf is NaN exactly where the trial finished"
    worst = 0.0
    for colour, own, other in ((1, gw_cpu, gb_cpu), (-1, gb_cpu, gw_cpu)):
        net = own if own is not None else other
        sel = ~done & (want["stop_player"] == colour)
        if not sel.any():
            continue
        x = torch.from_numpy(np.ascontiguousarray(want["feat"][sel]))
        with torch.no_grad():
            v32 = net(x).double().numpy().reshape(-1)
            v64 = copy.deepcopy(net).double()(x.double()).numpy().reshape(-1)
        E = max(float(np.abs(v32 - v64).max()), float(np.spacing(np.float32(max(np.abs(v64).max(), 1e-30)))))
        err = float(np.abs(leaf[sel].astype(np.float64) - v64).max())
        print(f"{what}: colour {colour}: {int(sel.sum())} leaves, max |leaf - ref| = {err:.3e}, E = {E:.3e}")
        assert err <= TOL_FACTOR * E, (what, colour, err, E)
        worst = max(worst, err)
    return worst


CASES = [(0, "all36", H128, H17), (1000, "nodoubles", H1, H128), (0, "nodoubles", H128, None),
         (1000, "all36", None, H1)]


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("id_base,dice_mode,white,black", CASES,
                         ids=lambda v: v if isinstance(v, (int, str)) else ("random" if v is None else f"H{v[0]}"))
def test_integer_outputs_equal_the_rollout_oracle(rules, id_base, dice_mode, white, black):
    state, t, trials, max_plies = seven_roots(), 4, 5, 12
    (gw, cw), (gb, cb) = twins(white), twins(black)
    want = oracle_run(rules, state, t, trials, max_plies, gw, gb, id_base=id_base, dice_mode=dice_mode, stop_feat=True)
    got = run_playout(rules, state, t, trials, max_plies, gw, gb, id_base=id_base, dice_mode=dice_mode, leaf=True)
    assert_integers_equal(got, want, f"{rules} id_base {id_base} {dice_mode}")
    # the inputs hold both ends: the endgames finish at once, the start position cannot in 12 plies
    assert want["done"][3:].any() and not want["done"][0].any()
    assert np.array_equal(np_(got["res"].finished), want["sums"][:, 0])
    check_leaf(got, want, cw, cb, f"{rules} id_base {id_base} {dice_mode}")


@pytest.mark.parametrize("rules", RULES)
def test_a_finishing_case(rules):
    """Late races and the endgames: the oracle shows every trial finished."""
    state, trials, max_plies = concat(late_races(), endgames()), 8, 40
    (gw, _), (gb, _) = twins(H80), twins(H17)
    want = oracle_run(rules, state, 0, trials, max_plies, gw, gb)
    assert want["done"].all() and (want["sums"][:, 0] == trials).all()  # the oracle first
    assert want["length"][:4].max() > 1  # the races take more than one ply
    got = run_playout(rules, state, 0, trials, max_plies, gw, gb, leaf=True)
    assert (got["sums"][:, 0] == trials).all()
    assert_integers_equal(got, want, rules)
    assert np.isnan(got["leaf"]).all()
    res = got["res"]
    mean = np_(res.mean())
    assert np.allclose(mean, want["outcome"].astype(np.float64).mean(1))
    sd = want["outcome"].astype(np.float64).std(1, ddof=1) / np.sqrt(trials)
    assert np.allclose(np_(res.stderr()), sd)


# Measured on one MI355X with these nets and this seed (docs/MEASUREMENT_LOG.md M.39): the longest of the 64
# games from the start position takes 121 plies under REF2 and 107 under FULL4.  The oracle runs ORACLE_PLIES
# plies; the playout's max_plies is the largest first-terminal ply it shows plus 10 % (134 and 118).
ORACLE_PLIES = 300


@pytest.mark.parametrize("rules", RULES)
def test_a_whole_game_from_the_start_position(rules):
    state, trials = start_position(), 64
    (gw, _), (gb, _) = twins(H80), twins(H17)
    want = oracle_run(rules, state, 0, trials, ORACLE_PLIES, gw, gb)
    assert want["done"].all(), "a game of the oracle's did not end: raise ORACLE_PLIES"
    longest = int(want["length"].max())
    max_plies = longest + (longest + 9) // 10
    print(f"{rules}: the longest of {trials} games takes {longest} plies; max_plies {max_plies}")
    got = run_playout(rules, state, 0, trials, max_plies, gw, gb)
    assert np.array_equal(got["sums"], want["sums"])
    assert_integers_equal(got, want, rules)


def test_full4_more_trials_than_waves_gives_the_same_bits():
    """10 trials on 3 pieces of scratch against a full-size scratch; trial 5 is
    big_state() (2,065 rows under 1-1: a level past the 256-node tier) on an
    id whose first roll is 1-1."""
    rules, trials, max_plies = "full4", 5, 6
    probe = make_env(4096, rules)
    first = np_(probe.dice())
    ones = np.flatnonzero((first == 1).all(1))
    ones = ones[ones >= trials]
    assert len(ones), "no env of the probe rolls 1-1 first: choose another seed"
    id_base = int(ones[0]) - trials  # trial q = 5, the big root's first, has that id
    big = big_state()
    state = concat(start_position(), (big["board"][None], big["off"][None], big["ft"][None],
                                      np.array([big["player"]], np.int8)))
    (gw, _), (gb, _) = twins(H80), twins(H17)
    # the oracle env's trial 5 does see 1-1 on big_state(): BIG_ROWS rows
    chk = make_env(2 * trials, rules, id_base=id_base)
    chk.set_state(*(torch.as_tensor(np.repeat(a, trials, axis=0)).to(chk.device) for a in state))
    assert np_(chk.dice())[trials].tolist() == [1, 1]
    aft = chk.turn_afterstates(feat=False)
    assert int(np.diff(np_(aft.offsets))[trials]) == BIG_ROWS
    few = run_playout(rules, state, 0, trials, max_plies, gw, gb, id_base=id_base, leaf=True,
                      scratch=probe.turn_value_rollout_scratch(3))
    full = run_playout(rules, state, 0, trials, max_plies, gw, gb, id_base=id_base, leaf=True,
                       scratch=probe.turn_value_rollout_scratch(2 * trials))
    for k in ("sums", "outcome", "length"):
        assert np.array_equal(few[k], full[k]), k
    assert np.array_equal(few["leaf"].view(np.uint32), full["leaf"].view(np.uint32))
    want = oracle_run(rules, state, 0, trials, max_plies, gw, gb, id_base=id_base)
    assert_integers_equal(few, want, "3 pieces")
    chk.close()
    probe.close()


@pytest.mark.parametrize("rules", RULES)
def test_common_dice_equals_the_single_root_calls(rules):
    state, t, trials, max_plies = seven_roots(), 2, 5, 12
    (gw, _), (gb, _) = twins(H128), twins(H17)
    many = run_playout(rules, state, t, trials, max_plies, gw, gb, id_base=40, common_dice=True, leaf=True)
    plain = run_playout(rules, state, t, trials, max_plies, gw, gb, id_base=40, leaf=True)
    for i in range(len(state[3])):
        one_state = tuple(a[i:i + 1] for a in state)
        one = run_playout(rules, one_state, t, trials, max_plies, gw, gb, id_base=40, leaf=True)
        for k in ("sums", "outcome", "length"):
            assert np.array_equal(many[k][i:i + 1], one[k]), (i, k)
        assert np.array_equal(many["leaf"][i:i + 1].view(np.uint32), one["leaf"].view(np.uint32)), i
    # and root 0 is the plain call's root 0; a later root has other dice there
    assert np.array_equal(many["length"][0], plain["length"][0])
    assert not np.array_equal(many["leaf"][1:3].view(np.uint32), plain["leaf"][1:3].view(np.uint32))


@pytest.mark.parametrize("rules", RULES)
def test_the_calling_handle_is_untouched(rules):
    env = make_env(33, rules, seed=5, id_base=2, max_steps=1000)
    (gw, _), _ = twins(H80), None
    if rules == "full4":
        env.turn_value_rollout(5, gw)
    else:
        env.value_rollout(5, gw)
    before = ({k: np_(v) for k, v in env.get_state().items()}, np_(env.stats()), int(env.ply))
    res = env.playout(env.get_state(), 3, gw, max_plies=9, seed=1, leaf=True, per_trial=True)
    assert np_(res.plies).sum() > 0
    after = ({k: np_(v) for k, v in env.get_state().items()}, np_(env.stats()), int(env.ply))
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_graph_capture_replays_and_reads_the_weights_in_place(rules):
    state, trials, max_plies = concat(start_position(), late_races()), 4, 6
    env = make_env(2, rules, seed=3, max_steps=1000)
    net = copy.deepcopy(make_net(*H80)).to(env.device)
    net.pack()
    roots = env.state_records(*state)
    out = env.playout(roots, trials, net, max_plies=max_plies, seed=SEED, per_trial=True, leaf=True)  # (makes scratch)
    torch.cuda.synchronize()
    eager = {k: np_(getattr(out, k)).copy() for k in ("sums", "outcome", "length", "leaf")}
    out.sums.fill_(-7)
    out.leaf.fill_(0.0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            env.playout(roots, trials, net, max_plies=max_plies, seed=SEED, per_trial=True, leaf=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):  # the sums do not accumulate from replay to replay
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert np.array_equal(np_(getattr(out, k)).view(np.uint8), eager[k].view(np.uint8)), k
    # new weights in place: the replay reads them (the start position's leaves move; the integer outputs equal
    # the oracle's under the new net)
    with torch.no_grad():
        other = make_net(*H80[:3], 9).to(env.device)
        for p, q in zip(net.parameters(), other.parameters()):
            p.copy_(q)
    net.pack()
    g.replay()
    torch.cuda.synchronize()
    leaf = np_(out.leaf)
    assert not np.isnan(leaf[0]).any() and (leaf[0] != eager["leaf"][0]).all()
    want = oracle_run(rules, state, 0, trials, max_plies, net, net)
    assert np.array_equal(np_(out.sums), want["sums"]) and np.array_equal(np_(out.length), want["length"])
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_state_records_are_the_rollouts_records(rules):
    state, t, trials = seven_roots(), 5, 1
    (gw, _), _ = twins(H17), None
    want = oracle_run(rules, state, t, trials, 1, gw, gw)
    caller = make_env(1, rules)
    rec = caller.state_records(*state, t=t)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (7, 8) and rec.data_ptr() % 16 == 0
    assert np.array_equal(np_(rec), want["records0"])
    # a get_state()-style dict is packed the same way (t = 0)
    st = dict(board=state[0], off=state[1], first_turn=state[2], player=state[3])
    a = caller.playout(st, 2, gw, max_plies=3, per_trial=True)
    b = caller.playout(caller.state_records(*state, t=0), 2, gw, max_plies=3, per_trial=True)
    assert np.array_equal(np_(a.sums), np_(b.sums)) and np.array_equal(np_(a.length), np_(b.length))
    caller.close()


def test_playout_values_is_the_one_net_mean():
    from gym_narde.value_play import playout_values

    state = concat(late_races(), endgames())
    (gw, _), _ = twins(H80), None
    env = make_env(1, "ref2")
    mean, err = playout_values(env, env.state_records(*state), gw, 8, max_plies=40, seed=SEED)
    want = oracle_run("ref2", state, 0, 8, 40, gw, gw)
    assert np.allclose(np_(mean), want["outcome"].astype(np.float64).mean(1))
    assert mean.dtype == torch.float64 and err.shape == mean.shape
    env.close()
