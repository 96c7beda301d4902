"""The FULL4 two-ply lookahead's reference pipeline,
shared by tests/test_turn_lookahead_cpu.py (the replies from enumerate_turns
over the C oracle) and tests/test_gpu_turn_lookahead.py (the replies from
VecNardeEnv.scored_turn_afterstates on a second env of the rows' records).
Test helper, not a test.

The rolls are the 21 unordered ones a <= b, a outer, b inner, a double of
weight 1 and any other of weight 2 (36 in all); NODOUBLES: the 15 unequal
ones.  The weighted mean goes through tests/lookahead_ref.py's two_ply with
every roll listed as often as its weight, which is the same number.
"""
import numpy as np

import lookahead_ref as LR
import oracle as O
import turn_afterstates_ref as R

ROLLS = [(a, b) for a in range(1, 7) for b in range(a, 7)]
WEIGHTS = [1 if a == b else 2 for a, b in ROLLS]


def rolls_of(dice_mode="all36"):
    """Indices into ROLLS of the dice mode's rolls."""
    return [k for k, (a, b) in enumerate(ROLLS) if dice_mode == "all36" or a != b]


def _popcount_below(mask, p):
    """Bits of mask below bit p (p < 0: none)."""
    mask = np.asarray(mask, np.uint64)
    p = np.clip(np.asarray(p, np.int64), 0, 24).astype(np.uint64)
    low = mask & ((np.uint64(1) << p) - np.uint64(1))
    return sum(((low >> np.uint64(q)) & np.uint64(1)).astype(np.int64) for q in range(24))


def oracle_step(board, off, ft, player, dice, play):
    """narde_step_full's position after `play` (n,4,2) int8 on the C oracle:
    or_full4_turn driven to the play by its pick words (entry i of a C_k of
    nc entries: the word ceil(i 2^32 / nc)), then the mover change unless the
    game ended.  An all -1 play is the pass where the turn has M = 0 (the
    oracle cannot play nothing where M > 0: such a row of the result is not
    that step's and its max_dice says so).  Returns a dict board, off,
    first_turn, player, reward, done, max_dice."""
    n = len(player)
    words = np.zeros((n, 4), np.uint32)
    play = np.asarray(play, np.int8)
    dh = np.asarray(dice, np.int64).max(1)
    for k in range(4):
        r = O.full4_turn(board, off, ft, player, dice, words)
        on = (play[:, k, 0] >= 0) & (r["max_dice"] > k)
        if not on.any():
            break
        mh, ml = r["cmask"][:, k, 0], r["cmask"][:, k, 1]
        src, die = play[:, k, 0].astype(np.int64), play[:, k, 1].astype(np.int64)
        high = (die == dh) & (((mh.astype(np.int64) >> np.clip(src, 0, 23)) & 1) == 1)
        idx = np.where(high, _popcount_below(mh, src), _popcount_below(mh, 24) + _popcount_below(ml, src))
        nc = np.maximum(_popcount_below(mh, 24) + _popcount_below(ml, 24), 1)
        w = ((idx.astype(np.uint64) << np.uint64(32)) + (nc - 1).astype(np.uint64)) // nc.astype(np.uint64)
        words[on, k] = w[on].astype(np.uint32)
    r = O.full4_turn(board, off, ft, player, dice, words)
    # the oracle played what the rows say
    m = r["max_dice"].astype(np.int64)
    for k in range(4):
        live = (m > k) & (play[:, 0, 0] >= 0)
        assert np.array_equal(r["played"][live, k], play[live, k]), k
    done = r["done"].astype(bool)
    return dict(board=r["board"], off=r["off"], first_turn=r["first_turn"], reward=r["reward"], done=done,
                player=np.where(done, player, -np.asarray(player)).astype(np.int8), max_dice=r["max_dice"])


def reference_case(st, dice_mode="all36", both_orders=False):
    """st: a dict board, off, ft, player, dice.  The first-ply rows over the
    oracle, their records by the oracle's step, and per roll of the dice mode
    the replies of the non-terminal rows with what a pass leaves.
    both_orders: the reply sets of (b, a) as well, under "swapped"."""
    ref = R.enumerate_turns(st["board"], st["off"], st["ft"], st["player"], st["dice"])
    e = ref["row_env"]
    stp = oracle_step(st["board"][e], st["off"][e], st["ft"][e], st["player"][e], st["dice"][e], ref["play"])
    assert np.array_equal(stp["board"], ref["board"]) and np.array_equal(stp["player"], ref["player"])
    assert np.array_equal(stp["reward"], ref["reward"])
    live = ref["reward"] == 0
    rec = tuple(np.ascontiguousarray(stp[k][live]) for k in ("board", "off", "first_turn", "player"))
    n = int(live.sum())
    ks = rolls_of(dice_mode)
    replies, swapped = [], []
    for k in ks:
        a, b = ROLLS[k]
        d = np.tile(np.array([a, b], np.uint8), (n, 1))
        rep = R.enumerate_turns(*rec, d)
        # a pass: what the step with an all -1 play leaves
        ps = oracle_step(*rec, d, np.full((n, 4, 2), -1, np.int8))
        rep.update(pass_feat=O.tesauro198(ps["board"], ps["off"], ps["player"]), pass_reward=ps["reward"],
                   pass_player=ps["player"], pass_board=ps["board"], pass_off=ps["off"], pass_ft=ps["first_turn"],
                   pass_max_dice=ps["max_dice"])
        replies.append(rep)
        if both_orders and a != b:
            swapped.append((k, R.enumerate_turns(*rec, np.ascontiguousarray(d[:, ::-1]))))
    return dict(ref=ref, live=live, rec=rec, replies=replies, ks=ks, ft=stp["first_turn"], swapped=swapped)


def two_ply_weighted(net, replies, ks, black):
    """LR.two_ply with the weighted mean: replies[i] is roll ROLLS[ks[i]].
    Returns (fp64 values (R,), fp32 values (R,), per roll m in fp64 (R, len(ks)))."""
    listed, first = [], []
    for rep, k in zip(replies, ks):
        first.append(len(listed))
        listed += [rep] * WEIGHTS[k]
    v64, v32, m64 = LR.two_ply(net, listed, black)
    return v64, v32, m64[:, first]


error_bound = LR.error_bound

# The two overflow tiers of the reply walk (found with enumerate_turns;
# tests/test_turn_lookahead_cpu.py asserts the counts).  Black to move with 14
# checkers on point 0 and one on point 2, dice 6-2, white's singles as listed.
# Slab tier: big_state()'s white singles; black's one row leaves big_state()
# to white, whose 1-1 reply has 2,065 rows (a level above 2,048) and whose
# other doubles have 726 .. 1,967.  LDS tier: the first ten of those singles;
# four rows, whose replies' largest levels lie in 257 .. 2,048 on 1-1 and 2-2.
TIER_SLAB_POINTS = R.BIG_POINTS
TIER_LDS_POINTS = R.BIG_POINTS[:10]


def tier_state(points):
    board = np.zeros(24, np.int8)
    board[list(points)] = 1
    board[0], board[2] = -14, -1
    return dict(board=board[None], off=np.array([[15 - len(points), 0]], np.uint8), ft=np.zeros((1, 2), np.uint8),
                player=np.array([-1], np.int8), dice=np.array([[6, 2]], np.uint8))
