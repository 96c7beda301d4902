"""Reference enumerator of FULL4 whole-turn afterstates, built only on
oracle.full4_turn (or_full4_turn, oracle/narde_oracle.c), and the shared
state set of the turn-afterstate tests.

A play is a sequence of sub-moves, each an entry of the oracle's C_k for the
prefix before it, of length M.  The enumerator walks the prefixes level by
level: entry i of a C_k of nc entries is selected with the pick word
ceil(i * 2^32 / nc) (the smallest w with mulhi(w, nc) == i), the call's
cmask[k] is the C_k of the next level, and a prefix of length M is a play.
Plays come out in lexicographic order of their entries (list order: higher
die first, source ascending); the rows of a state are the distinct final
(board, off) in first-seen order.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O

# white singles on 3, 5, 6, 7, 9, 11, 12, 13, 14, 17, 18, 20, 21, 22, 23, black's 15
# on point 0, white to move, dice 1-1: 2,065 rows from 40,426 plays
BIG_POINTS = (3, 5, 6, 7, 9, 11, 12, 13, 14, 17, 18, 20, 21, 22, 23)
BIG_ROWS, BIG_PLAYS = 2065, 40426


def big_state():
    board = np.zeros(24, np.int8)
    board[list(BIG_POINTS)] = 1
    board[0] = -15
    return dict(board=board, off=np.zeros(2, np.uint8), ft=np.zeros(2, np.uint8), player=np.int8(1),
                dice=np.array([1, 1], np.uint8))


def _popcount24(m):
    m = np.asarray(m, np.uint32)
    return sum(((m >> np.uint32(p)) & np.uint32(1)).astype(np.int64) for p in range(24))


def _full4_turn(board, off, ft, player, dice, words, chunk=4096):
    """O.full4_turn over slices on a few threads (the C call releases the GIL)."""
    n = len(player)
    if n <= chunk:
        return O.full4_turn(board, off, ft, player, dice, words)
    cuts = [slice(a, min(a + chunk, n)) for a in range(0, n, chunk)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        parts = list(ex.map(lambda c: O.full4_turn(board[c], off[c], ft[c], player[c], dice[c], words[c]), cuts))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def enumerate_turns(board, off, ft, player, dice):
    """Rows of every state.  Returns a dict: offsets (n + 1,), plays (n,) --
    the number of plays --, max_dice (n,), and per row: row_env, play
    (R,4,2) int8 (from, die), -1 padded, board, off, player (after the
    flip; not flipped after a terminal turn), reward, feat (R,198), obs
    (R,24) -- the board as the player to move sees it."""
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    board, off, ft, player, dice = c(board, np.int8), c(off, np.uint8), c(ft, np.uint8), c(player, np.int8), c(dice, np.uint8)
    n = board.shape[0]
    ok = ((dice >= 1) & (dice <= 6)).all(1)
    # the live prefixes: (state, words so far), state-major, lexicographic
    st = np.flatnonzero(ok).astype(np.int64)
    words = np.zeros((len(st), 4), np.uint32)
    fin_keys = ("board", "off", "played", "reward", "done")
    done = {k: [] for k in ("state", "words") + fin_keys}
    max_dice = np.zeros(n, np.int8)
    for k in range(5):
        if not len(st):
            break
        r = _full4_turn(board[st], off[st], ft[st], player[st], dice[st], words)
        M = r["max_dice"].astype(np.int64)
        if k == 0:
            max_dice[st] = r["max_dice"]
        # a prefix of length M is a play, and this call has carried it out
        fin = (M == k) & (M > 0)
        done["state"].append(st[fin])
        done["words"].append(words[fin])
        for key in fin_keys:
            done[key].append(r[key][fin])
        live = np.flatnonzero(M > k)
        if k == 4 or not len(live):
            break
        # C_k of each live prefix: its size is all the selection needs (entry
        # i of nc is picked by the word ceil(i * 2^32 / nc))
        nc = _popcount24(r["cmask"][live, k, 0]) + _popcount24(r["cmask"][live, k, 1])
        rep = np.repeat(np.arange(len(live)), nc)
        i = np.arange(len(rep), dtype=np.int64) - np.repeat(np.cumsum(nc) - nc, nc)
        ncr = nc[rep]
        st = st[live][rep]
        words = words[live][rep].copy()
        words[:, k] = ((i.astype(np.uint64) << np.uint64(32)) + (ncr - 1).astype(np.uint64)) // ncr.astype(np.uint64)
    # lexicographic play order within a state: under a common prefix the
    # word grows with the entry index, so the words sort as the entries do
    ds = np.concatenate(done["state"]) if done["state"] else np.zeros(0, np.int64)
    dw = np.concatenate(done["words"]) if done["words"] else np.zeros((0, 4), np.uint32)
    plays = np.bincount(ds, minlength=n).astype(np.int64)
    keep = np.zeros(len(ds), bool)
    if len(ds):
        order = np.lexsort((dw[:, 3], dw[:, 2], dw[:, 1], dw[:, 0], ds))
        ds = ds[order]
        r = {key: np.concatenate(done[key])[order] for key in fin_keys}
        # the first play of each distinct (state, board, off)
        ident = np.concatenate([ds[:, None].view(np.uint8).reshape(len(ds), 8), r["board"].view(np.uint8), r["off"]], 1)
        _, first = np.unique(np.ascontiguousarray(ident).view([("", np.uint8, ident.shape[1])]).ravel(), return_index=True)
        keep[first] = True
    counts = np.bincount(ds[keep], minlength=n)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    out = dict(offsets=offsets, plays=plays, max_dice=max_dice, row_env=ds[keep].astype(np.int32))
    if len(ds):
        out["play"] = r["played"][keep]
        out["board"], out["off"], out["reward"] = r["board"][keep], r["off"][keep], r["reward"][keep]
        done = r["done"][keep].astype(bool)
        out["player"] = np.where(done, player[ds[keep]], -player[ds[keep]]).astype(np.int8)
    else:
        out["play"] = np.zeros((0, 4, 2), np.int8)
        out["board"], out["off"] = np.zeros((0, 24), np.int8), np.zeros((0, 2), np.uint8)
        out["reward"], out["player"] = np.zeros(0, np.int8), np.zeros(0, np.int8)
    out["feat"] = O.tesauro198(out["board"], out["off"], out["player"]) if len(out["board"]) else np.zeros((0, 198), np.float32)
    out["obs"] = np.where((out["player"] == 1)[:, None], out["board"], -np.roll(out["board"], 12, axis=1)).astype(np.int32)
    return out


def selfplay_states(n=64, plies=120, every=4, seed=0):
    """The state before every `every`-th of `plies` FULL4 self-play plies
    with that ply's dice (O.SelfPlay(n, seed) under run_full)."""
    sp = O.SelfPlay(n, seed=seed)
    sp.reset(0)
    out = dict(board=[], off=[], ft=[], player=[], dice=[])
    for p in range(plies):
        snap = (sp.board.copy(), sp.off.copy(), sp.ft.copy(), sp.player.copy())
        rec = sp.run_full(1)
        if p % every == 0:
            for k, v in zip(("board", "off", "ft", "player"), snap):
                out[k].append(v)
            out["dice"].append(rec["dice"][0].copy())
    return {k: np.concatenate(v) for k, v in out.items()}


def start_states():
    """The start position (white to move) under all 36 dice: the first-turn
    3-3 / 4-4 / 6-6 head rule."""
    board = np.zeros((36, 24), np.int8)
    board[:, 23], board[:, 11] = 15, -15
    dice = np.array([(a, b) for a in range(1, 7) for b in range(1, 7)], np.uint8)
    return dict(board=board, off=np.zeros((36, 2), np.uint8), ft=np.ones((36, 2), np.uint8),
                player=np.ones(36, np.int8), dice=dice)


def _mk(rows):
    """rows: (white {point: n}, black {point: n}, off (w, b), ft (w, b), player, dice)"""
    n = len(rows)
    s = dict(board=np.zeros((n, 24), np.int8), off=np.zeros((n, 2), np.uint8), ft=np.zeros((n, 2), np.uint8),
             player=np.zeros(n, np.int8), dice=np.zeros((n, 2), np.uint8))
    for i, (w, b, off, ft, player, dice) in enumerate(rows):
        for p, c in w.items():
            s["board"][i, p] = c
        for p, c in b.items():
            s["board"][i, p] = -c
        s["off"][i], s["ft"][i], s["player"][i], s["dice"][i] = off, ft, player, dice
    return s


def edge_states():
    """Bear-off endings (terminal rows of reward 1 and 2), two-dice turns with
    M = 1 for each die, passes, a bad die."""
    return _mk([
        # white bears its last two off: black has borne off -> reward 1; not -> 2
        ({0: 1, 2: 1}, {12: 10}, (13, 5), (0, 0), 1, (3, 1)),
        ({0: 1, 2: 1}, {12: 15}, (13, 0), (0, 0), 1, (3, 1)),
        ({1: 2}, {13: 15}, (13, 0), (0, 0), 1, (2, 2)),
        ({3: 1}, {14: 3}, (14, 12), (0, 0), 1, (6, 5)),
        # black to move (absolute coordinates: black's home is 12..17)
        ({2: 15}, {12: 1, 13: 1}, (0, 13), (0, 0), -1, (2, 1)),
        # M = 1, the higher die only: 22 black blocks the 1, and 16 black the 1 after the 6
        ({23: 1}, {22: 1, 16: 1, 10: 13}, (14, 0), (0, 0), 1, (6, 1)),
        # M = 1, the lower die only: 17 black blocks the 6, and 16 black the 6 after the 1
        ({23: 1}, {17: 1, 16: 1, 10: 13}, (14, 0), (0, 0), 1, (6, 1)),
        # M = 1, either die alone but not both: the higher die's move is the row
        ({23: 1}, {16: 1, 10: 14}, (14, 0), (0, 0), 1, (6, 1)),
        # a pass: both landings blocked
        ({23: 1}, {17: 1, 22: 1, 10: 13}, (14, 0), (0, 0), 1, (6, 1)),
        # a die outside 1..6: no row
        ({23: 15}, {11: 15}, (0, 0), (1, 1), 1, (0, 3)),
        ({23: 15}, {11: 15}, (0, 0), (1, 1), 1, (7, 7)),
        # doubles that stop short (M = 2 of 4)
        ({23: 1}, {17: 1, 10: 14}, (14, 0), (0, 0), 1, (2, 2)),
    ])


def golden_states(g):
    """Every state of tests/golden/full4.npz."""
    return dict(board=g["board"], off=g["off"], ft=g["ft"], player=g["player"], dice=g["dice"])


def concat(*sets):
    return {k: np.concatenate([np.asarray(s[k]).reshape((-1,) + np.asarray(s[k]).shape[1:]) if np.asarray(s[k]).ndim else
                               np.asarray(s[k]).reshape(1) for s in sets]) for k in ("board", "off", "ft", "player", "dice")}


def big_states():
    b = big_state()
    return {k: np.asarray(v)[None] for k, v in b.items()}
