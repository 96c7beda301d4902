"""The one-launch rollouts (k_value_rollout, k_turn_value_rollout) and the
playouts on positions play from the start position does not reach in a few
plies (tests/fuzz_positions.py: run-heavy boards and bear-off endgames), placed
so that the run-heavy boards sit on the env ids whose own first roll is a
double (place_for_rolls; tests/test_rollout_fuzz_cpu.py asserts on the oracle
what the placed set holds).

What the positions are for:
  * more than 64 rows an env: the second 64-row chunk of the wave's choice,
    row ordinals above 63, a lane's best carried from one chunk to the next
    into the merge; an explore ply whose drawn ordinal is 64 or more;
  * under FULL4 more than 256 rows: the slab walk inside a launch, and with
    three pieces of scratch several overflowing envs through one wave's slab
    piece, one after another, after other envs have left their keys in its LDS
    frontier;
  * no-row plies and terminal rows that nobody placed by hand;
  * the feature staging's branches for stacks and borne-off counts.

The yardstick is the replay modules' own: the composed path --
scored_afterstates / scored_turn_afterstates, the pick, the step -- walked per
ply on a second env, and their judgement unchanged (the recorded action a row;
the float64 reference's arg-best where its gap exceeds 8 E, else within 8 E; at
most 1 % of greedy plies exempt; values within 8 E; reward, flags, final state
and statistics the stepped twin's).  The playouts are held against the rollouts
on the same roots, as tests/test_gpu_value_playout.py holds them.  Every case
asserts from the replay's counters that it ran what it was built for.
"""
import numpy as np
import pytest

from fuzz_positions import first_rolls, place_for_rolls, turn_states
from test_rollout_fuzz_cpu import (B, CHUNK, COMMON_BASE, ENV0, FRONT, ID_BASE, N, PLAYOUT_SEED, POS_SEED, SEED, TRIALS,
                                   playout_roots)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_td_window as TW  # noqa: E402
import test_gpu_turn_value_rollout as TR  # noqa: E402
import test_gpu_value_playout as VP  # noqa: E402
import test_gpu_value_rollout as VR  # noqa: E402
from test_gpu_value_rollout import H1, H17, H80, H128, np_  # noqa: E402

RULES = ("ref2", "full4")
PLIES = 3
STATE = ("board", "off", "ft", "player")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def state():
    """The placed set; the device's first rolls are the oracle's it was placed for."""
    assert (VR.SEED, VR.ENV0, TR.SEED, TR.ENV0, VP.SEED) == (SEED, ENV0, SEED, ENV0, PLAYOUT_SEED)
    first = first_rolls(B, SEED, ENV0)
    for make in (VR.make_env, TR.make_env):
        probe = make(B)
        assert np.array_equal(np_(probe.dice()), first)
        probe.close()
    st = place_for_rolls(turn_states(B, POS_SEED), first)
    return tuple(st[k] for k in STATE)


def run(rules, *args, **kw):
    """(J, bufs) of the rules' replay module's run_case."""
    if rules == "full4":
        return TR.run_case(*args, **kw)
    return VR.run_case(*args, **kw), None


def counters(J, what):
    verr = max(J["verr"]) if J["verr"] else 0.0
    print(f"{what}: most rows {J['most_rows']}, greedy plies above {CHUNK} rows {J['greedy_above_64']}, plies above {FRONT} "
          f"{J['above_256']}, explore ordinals >= 64 {J['explore_ordinal_64']}, no-row {J['norow']}, terminal picks "
          f"{J['terminal_pick']}, resets {J['resets']}, max |value - ref| {verr:.3e}")


def ran_what_it_was_built_for(J, rules, what):
    counters(J, what)
    assert J["greedy_above_64"] > 0 and J["most_rows"] > CHUNK
    assert rules != "full4" or (J["above_256"] > 0 and J["most_rows"] > FRONT)
    assert J["norow"] > 0 and J["terminal_pick"] > 0 and J["resets"] > 0


@pytest.fixture(scope="module")
def full4_two_nets(state):
    """The FULL4 two-net greedy case on a scratch piece an env: (J, bufs), once a module."""
    return TR.run_case(B, PLIES, H128, H17, state=state, what="full4 H 128 white, H 17 black")


# ---------------------------------------------------------------- the rollouts, judged

@pytest.mark.parametrize("rules", RULES)
def test_greedy_one_net(rules, state):
    what = f"{rules} H 80"
    J, _ = run(rules, B, PLIES, H80, state=state, what=what)
    assert J["greedy"] + J["norow"] == B * PLIES
    ran_what_it_was_built_for(J, rules, what)


@pytest.mark.parametrize("rules", RULES)
def test_greedy_two_different_nets(rules, state, request):
    what = f"{rules} H 128 white, H 17 black"
    if rules == "full4":
        J, _ = request.getfixturevalue("full4_two_nets")
    else:
        J, _ = run(rules, B, PLIES, H128, H17, state=state, what=what)
    assert J["greedy"] + J["norow"] == B * PLIES
    ran_what_it_was_built_for(J, rules, what)


@pytest.mark.parametrize("rules", RULES)
def test_the_degenerate_net(rules, state):
    what = f"{rules} H 1"
    J, _ = run(rules, B, PLIES, H1, state=state, what=what)
    assert J["greedy"] + J["norow"] == B * PLIES
    ran_what_it_was_built_for(J, rules, what)


@pytest.mark.parametrize("rules", RULES)
def test_epsilon_draws_a_row_past_the_first_chunk(rules, state):
    what = f"{rules} epsilon 0.3"
    J, _ = run(rules, B, PLIES, H80, eps=0.3, state=state, what=what)
    assert J["explored"] > 60 and J["greedy"] > 180  # 0.3 and 0.7 of 384 plies, less four standard deviations
    assert J["explore_ordinal_64"] >= 1, "no explore ply drew an ordinal of 64 or more: choose another tag"
    ran_what_it_was_built_for(J, rules, what)


@pytest.mark.parametrize("rules", RULES)
@pytest.mark.parametrize("random_colour", ["black", "white"])
def test_one_colour_random(rules, random_colour, state):
    """The random turn runs inside the rollout wave, on doubles-heavy boards;
    the other colour's plies are judged (the CPU test: each colour has rows
    above 64 and 256, a no-row env and a terminal row of its own)."""
    what = f"{rules} {random_colour} random"
    nets = (H80, None) if random_colour == "black" else (None, H17)
    J, _ = run(rules, B, PLIES, *nets, state=state, what=what)
    assert J["random"] > 100 and J["greedy"] > 100 and J["random"] + J["greedy"] + J["norow"] == B * PLIES
    ran_what_it_was_built_for(J, rules, what)


@pytest.mark.parametrize("rules", RULES)
def test_truncation_and_reset_inside_the_launch(rules, state):
    what = f"{rules} max_episode_steps 2"
    J, _ = run(rules, B, PLIES, H80, H17, max_steps=2, state=state, what=what)
    assert J["resets"] >= B  # every env's second ply is its episode's last
    ran_what_it_was_built_for(J, rules, what)


def test_full4_three_pieces_of_scratch_give_the_same_bits(state, full4_two_nets):
    """About 43 envs a wave, several slab walks a wave one after another:
    judged like every case, and every buffer the full-size scratch's bits.
    (Both runs' final states and statistics equal their stepped twins', which
    are the same calls on the same recorded plays.)"""
    what = "full4 H 128 white, H 17 black, 3 pieces of scratch"
    _, full = full4_two_nets
    J, few = TR.run_case(B, PLIES, H128, H17, state=state, what=what, scratch_waves=3)
    ran_what_it_was_built_for(J, "full4", what)
    assert J["above_256"] > 3  # more overflowing envs than waves
    TR.assert_same_bufs(few, full, what)


@pytest.mark.parametrize("rules", RULES)
def test_a_middle_game_reached_by_play(rules):
    """test_gpu_td_window.middle_game: 40 plies of self-play, elapsed counts
    staggered below max_episode_steps 44, eight envs one ply from winning."""
    what = f"{rules} middle game"
    env = TW.middle_game(rules, 65)
    st = {k: np_(v) for k, v in env.get_state().items()}
    env.close()
    mid = tuple(st[k] for k in ("board", "off", "first_turn", "player", "elapsed"))
    J, _ = run(rules, 65, 7, H80, H17, max_steps=44, state=mid, what=what)
    counters(J, what)
    assert J["greedy"] + J["norow"] == 65 * 7
    assert J["terminal_pick"] >= 8 and J["resets"] >= 65  # the eight win at once, every other env meets the TimeLimit within four plies


# ---------------------------------------------------------------- the playouts, from the same roots

MAX_PLIES = 4


def root_state(roots):
    return tuple(np.ascontiguousarray(roots[k]) for k in STATE)


def probe_rows(rules, st, rolls, id_base):
    """The trials' first rolls and row counts, from an env of the trials' ids."""
    chk = VP.make_env(N * TRIALS, rules, id_base=id_base)
    chk.set_state(*(torch.as_tensor(np.repeat(a, TRIALS, axis=0)).to(chk.device) for a in st))
    assert np.array_equal(np_(chk.dice()), rolls.reshape(-1, 2))
    aft = chk.turn_afterstates(feat=False) if rules == "full4" else chk.afterstates(feat=False)
    cnt = np.diff(np_(aft.offsets))
    chk.close()
    return cnt


@pytest.mark.parametrize("rules", RULES)
def test_playouts_equal_the_rollout_oracle(rules):
    roots, rolls = playout_roots()
    st = root_state(roots)
    cnt = probe_rows(rules, st, rolls, ID_BASE)
    print(f"{rules} playout roots: most rows {cnt.max()}, trials above {CHUNK} rows {(cnt > CHUNK).sum()}, above {FRONT} "
          f"{(cnt > FRONT).sum()}, no row {(cnt == 0).sum()}")
    assert (cnt > FRONT).sum() >= 4 if rules == "full4" else (cnt > CHUNK).sum() >= 4
    (gw, cw), (gb, cb) = VP.twins(H128), VP.twins(H17)
    want = VP.oracle_run(rules, st, 0, TRIALS, MAX_PLIES, gw, gb, id_base=ID_BASE, stop_feat=True)
    got = VP.run_playout(rules, st, 0, TRIALS, MAX_PLIES, gw, gb, id_base=ID_BASE, leaf=True)
    VP.assert_integers_equal(got, want, rules)
    assert want["done"].any() and not want["done"].all()  # endgames that finish, boards that cannot
    assert np.array_equal(np_(got["res"].finished), want["sums"][:, 0])
    VP.check_leaf(got, want, cw, cb, f"{rules} fuzz roots")


def test_full4_playouts_on_three_pieces_of_scratch():
    """Several different overflowing trials through one wave's slab piece."""
    rules = "full4"
    roots, rolls = playout_roots()
    st = root_state(roots)
    (gw, _), (gb, _) = VP.twins(H128), VP.twins(H17)
    probe = VP.make_env(1, rules)
    few = VP.run_playout(rules, st, 0, TRIALS, MAX_PLIES, gw, gb, id_base=ID_BASE, leaf=True,
                         scratch=probe.turn_value_rollout_scratch(3))
    full = VP.run_playout(rules, st, 0, TRIALS, MAX_PLIES, gw, gb, id_base=ID_BASE, leaf=True,
                          scratch=probe.turn_value_rollout_scratch(N * TRIALS))
    for k in ("sums", "outcome", "length"):
        assert np.array_equal(few[k], full[k]), k
    assert np.array_equal(few["leaf"].view(np.uint32), full["leaf"].view(np.uint32))
    want = VP.oracle_run(rules, st, 0, TRIALS, MAX_PLIES, gw, gb, id_base=ID_BASE)
    VP.assert_integers_equal(few, want, "3 pieces")
    probe.close()


@pytest.mark.parametrize("rules", RULES)
def test_common_dice_equals_the_single_root_calls(rules):
    """Every root on the ids COMMON_BASE, COMMON_BASE + 1 (1-1 both): each
    run-heavy root's numbers are those of a call with that root alone."""
    roots, _ = playout_roots()
    st = root_state(roots)
    common = first_rolls(TRIALS, PLAYOUT_SEED, COMMON_BASE)
    assert (common[:, 0] == common[:, 1]).all()
    (gw, _), (gb, _) = VP.twins(H128), VP.twins(H17)
    many = VP.run_playout(rules, st, 0, TRIALS, MAX_PLIES, gw, gb, id_base=COMMON_BASE, common_dice=True, leaf=True)
    heavy = np.flatnonzero(roots["heavy"])
    assert len(heavy) == N // 2
    for i in heavy:
        one_state = tuple(a[i:i + 1] for a in st)
        one = VP.run_playout(rules, one_state, 0, TRIALS, MAX_PLIES, gw, gb, id_base=COMMON_BASE, leaf=True)
        for k in ("sums", "outcome", "length"):
            assert np.array_equal(many[k][i:i + 1], one[k]), (i, k)
        assert np.array_equal(many["leaf"][i:i + 1].view(np.uint32), one["leaf"].view(np.uint32)), i
