"""The positions tests/test_gpu_rollout_fuzz.py replays the one-launch
rollouts and the playouts on, checked on the oracle before any kernel is in the
picture.

A rollout draws its own dice: the roll an env sees at ply counter t depends on
the seed, the env id and t, not on the position.  fuzz_positions.place_for_rolls
therefore puts the run-heavy half of a turn_states() set first on the ids whose
first roll is a double -- a run-heavy board on a double is what outgrows the
64-row chunk and, under FULL4, the 256-node frontier.  The first rolls come from
the oracle (O.SelfPlay(B, seed, env0).reset(0), run(1)["dice"][0]; run_full
gives the same), the row counts from reference_afterstates and
turn_afterstates_ref.enumerate_turns.

Measured for turn_states(128, 808), seed 20251020, ids from 3 (21 of the 128
ids roll a double first): FULL4 32 envs above 64 rows, 8 above 256, the largest
548, 2 with no row, 2 terminal rows; REF2 7 above 64 (the largest 92), 2 with no
row, 2 terminal rows.  The tests assert floors, not these figures.
"""
import numpy as np
import pytest

import oracle as O
import turn_afterstates_ref as R
from fuzz_positions import first_rolls, place_for_rolls, turn_states
from test_afterstates_cpu import reference_afterstates

B, POS_SEED = 128, 808
SEED, ENV0 = 20251020, 3  # tests/test_gpu_value_rollout.py's and test_gpu_turn_value_rollout.py's
KEYS = ("board", "off", "ft", "player", "dice")
CHUNK, FRONT = 64, 256  # the rollouts' rows a chunk; kTurnFront


@pytest.fixture(scope="module")
def first():
    return first_rolls(B, SEED, ENV0)


@pytest.fixture(scope="module")
def placed(first):
    return place_for_rolls(turn_states(B, POS_SEED), first)


def test_first_rolls_are_both_drivers(first):
    sp = O.SelfPlay(B, SEED, ENV0)
    sp.reset(0)
    assert np.array_equal(sp.run_full(1)["dice"][0], first)
    assert first.shape == (B, 2) and first.min() >= 1 and first.max() <= 6
    dbl = first[:, 0] == first[:, 1]
    assert 8 <= dbl.sum() <= B // 2  # enough doubles to matter, fewer than the run-heavy half


def test_placement_is_a_permutation_with_the_run_heavy_half_on_the_doubles(first, placed):
    st = turn_states(B, POS_SEED)
    key = lambda s: sorted(bytes(np.concatenate([s["board"][i].view(np.uint8), s["off"][i], s["ft"][i],  # noqa: E731
                                                 s["player"][i:i + 1].view(np.uint8)])) for i in range(B))
    assert key(st) == key(placed)
    dbl = first[:, 0] == first[:, 1]
    assert placed["heavy"][dbl].all() and placed["heavy"].sum() == B // 2
    assert np.array_equal(placed["dice"], first)
    # in the set's order: its first positions on the doubles, the rest on the ids left
    assert np.array_equal(placed["board"][dbl], st["board"][:dbl.sum()])
    assert np.array_equal(placed["board"][~dbl], st["board"][dbl.sum():])
    # several trials an id: one double among them is enough
    rolls = np.stack([first, np.roll(first, 1, axis=0)], 1)
    two = place_for_rolls(st, rolls)
    either = (rolls[:, :, 0] == rolls[:, :, 1]).any(1)
    assert dbl.sum() < either.sum() <= B // 2 and two["heavy"][either].all() and two["heavy"].sum() == B // 2


def _floors(cnt, ref, player, above_chunk, above_front):
    assert (cnt > CHUNK).sum() >= above_chunk, (cnt > CHUNK).sum()
    assert (cnt > FRONT).sum() >= above_front, (cnt > FRONT).sum()
    assert (cnt == 0).sum() >= 1 and (ref["reward"] != 0).sum() >= 1
    # each colour on its own -- the cases with one colour random judge the other's plies only
    won = np.zeros(len(cnt), bool)
    won[ref["row_env"][ref["reward"] != 0]] = True
    for colour in (1, -1):
        m = player == colour
        assert (cnt[m] > CHUNK).any() and (cnt[m] == 0).any() and won[m].any(), colour
        assert not above_front or (cnt[m] > FRONT).any(), colour


def test_full4_floors(placed):
    ref = R.enumerate_turns(*(placed[k] for k in KEYS))
    cnt = np.diff(ref["offsets"])
    print(f"full4: above {CHUNK} rows {(cnt > CHUNK).sum()}, above {FRONT} {(cnt > FRONT).sum()}, largest {cnt.max()}, "
          f"no row {(cnt == 0).sum()}, terminal rows {(ref['reward'] != 0).sum()}")
    _floors(cnt, ref, placed["player"], 16, 4)
    # an env above the frontier has a run-heavy board and a double
    big = cnt > FRONT
    assert placed["heavy"][big].all() and (placed["dice"][big, 0] == placed["dice"][big, 1]).all()


def test_ref2_floors(placed):
    ref = reference_afterstates(*(placed[k] for k in KEYS))
    cnt = np.diff(ref["offsets"])
    print(f"ref2: above {CHUNK} rows {(cnt > CHUNK).sum()}, largest {cnt.max()}, no row {(cnt == 0).sum()}, "
          f"terminal rows {(ref['reward'] != 0).sum()}")
    _floors(cnt, ref, placed["player"], 4, 0)


# ---------------------------------------------------------------- the playouts' roots

PLAYOUT_SEED = 20251021  # tests/test_gpu_value_playout.py's
N, TRIALS, ID_BASE = 48, 2, 0
COMMON_BASE = 14  # ids 14 and 15 both roll 1-1 first under PLAYOUT_SEED: every root's two trials with common dice


def playout_roots(id_base=ID_BASE):
    """24 run-heavy and 24 endgame positions of the set, the run-heavy ones
    at the root indices one of whose trial ids (id_base + i * TRIALS + j) rolls
    a double first.  Returns (the placed dict, the (N, TRIALS, 2) first rolls)."""
    full = turn_states(B, POS_SEED)
    idx = np.concatenate([np.arange(N // 2), B // 2 + np.arange(N // 2)])
    sub = {k: np.asarray(full[k])[idx] for k in KEYS}
    rolls = first_rolls(N * TRIALS, PLAYOUT_SEED, id_base).reshape(N, TRIALS, 2)
    return place_for_rolls(sub, rolls), rolls


def trial_rows(roots, rolls, enumerate_fn):
    """Row counts of every trial's first ply, (N * TRIALS,)."""
    rep = [np.repeat(roots[k], TRIALS, axis=0) for k in ("board", "off", "ft", "player")]
    return np.diff(enumerate_fn(*rep, rolls.reshape(-1, 2))["offsets"])


def test_playout_roots_floors():
    """Measured: 14 of the 96 trial ids roll a double; FULL4 7 trials above
    256 rows (the largest 541) and 24 above 64; REF2 10 above 64; 4 with no
    row."""
    roots, rolls = playout_roots()
    dbl = (rolls[:, :, 0] == rolls[:, :, 1]).any(1)
    assert roots["heavy"][dbl].all() and roots["heavy"].sum() == N // 2
    full = trial_rows(roots, rolls, R.enumerate_turns)
    ref2 = trial_rows(roots, rolls, reference_afterstates)
    print(f"playout roots: full4 above {FRONT} rows {(full > FRONT).sum()}, above {CHUNK} {(full > CHUNK).sum()}, largest "
          f"{full.max()}; ref2 above {CHUNK} {(ref2 > CHUNK).sum()}, largest {ref2.max()}")
    assert (full > FRONT).sum() >= 4 and (ref2 > CHUNK).sum() >= 4
    assert (full == 0).any() and (ref2 == 0).any()
    # with common dice every root plays ids COMMON_BASE, COMMON_BASE + 1: doubles both
    common = first_rolls(TRIALS, PLAYOUT_SEED, COMMON_BASE)
    assert (common[:, 0] == common[:, 1]).all()
    both = np.broadcast_to(common, (N, TRIALS, 2))
    # (REF2 plays two sub-moves of a double: its rows above 64 come from two different dice)
    assert (trial_rows(roots, both, R.enumerate_turns)[roots["heavy"].repeat(TRIALS)] > FRONT).sum() >= 8
