"""Random positions for differential tests (test_gpu_fuzz.py,
test_full4_cpu.py, test_gpu_afterstate_fuzz.py, test_rollout_fuzz_cpu.py,
test_gpu_rollout_fuzz.py): run-heavy boards where the block rule decides and
bear-off endgames, placed for a random mover.  Test helper, not a test."""
import numpy as np
from test_oracle_golden import _prime_boards


def endgame_boards(n, seed):
    """Mover (positive, perspective) mostly home with some checkers off,
    a few stragglers outside; opponent on 1-3 points the mover leaves free."""
    rng = np.random.default_rng(seed)
    boards = np.zeros((n, 24), np.int8)
    off = np.zeros((n, 2), np.uint8)
    for i in range(n):
        k = int(rng.integers(0, 14))
        for _ in range(15 - k):
            p = int(rng.integers(0, 6)) if rng.random() < 0.85 else int(rng.integers(6, 14))
            boards[i, p] += 1
        free = np.nonzero(boards[i] == 0)[0]
        pts = rng.choice(free, size=min(int(rng.integers(1, 4)), len(free)), replace=False)
        opp = 15
        for j, p in enumerate(pts):
            c = opp if j == len(pts) - 1 else int(rng.integers(1, opp - (len(pts) - 1 - j) + 1))
            boards[i, p] = -c
            opp -= c
        off[i, 0] = k
    return boards, off


def random_positions(n, seed):
    """Half run-heavy, half endgame perspective positions, each placed on
    the absolute board for a random mover: white as is, black rotated
    (get_perspective_board(-1) = rotate_board, narde.py:16-17,31-34).
    Returns (board, off, first_turn, player, rng)."""
    rng = np.random.default_rng(seed)
    h = n // 2
    pb = _prime_boards(h, seed + 1)
    eb, eoff = endgame_boards(n - h, seed + 2)
    persp = np.concatenate([pb, eb])
    off = np.concatenate([np.zeros((h, 2), np.uint8), eoff])
    player = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    board = persp.copy()
    blk = player == -1
    board[blk] = -np.roll(persp[blk], 12, axis=1)
    off[blk] = off[blk][:, ::-1]
    ft = rng.integers(0, 2, (n, 2)).astype(np.uint8)
    return board, np.ascontiguousarray(off), ft, player, rng


def _rolls(rng, n, doubles):
    d0 = rng.integers(1, 7, n)
    d1 = np.where(rng.random(n) < doubles, d0, rng.integers(1, 7, n))
    return np.stack([d0, d1], 1).astype(np.uint8)


def turn_states(n, seed, doubles=0.5):
    """random_positions(n, seed) with a roll each, dice 1..6, a double with
    probability `doubles` (a run-heavy board on a double is what outgrows the
    turn kernels' 256-node frontier): the dict board, off, ft, player, dice
    of tests/turn_afterstates_ref.py."""
    board, off, ft, player, rng = random_positions(n, seed)
    dice = _rolls(rng, n, doubles)
    # endgame_boards leaves the opponent's 15 on the board, so a win there is
    # always worth 2: on half of the endgame states the opponent has borne
    # 1..14 off as well (taken from its points in ascending order), which
    # makes the win worth 1
    for i in range(n // 2, n):
        if rng.random() < 0.5:
            take = int(rng.integers(1, 15))
            opp = -int(player[i])
            for p in np.nonzero(board[i] * opp > 0)[0]:
                c = min(take, abs(int(board[i, p])))
                board[i, p] -= opp * c
                take -= c
                off[i, 0 if opp == 1 else 1] += c
    return dict(board=board, off=off, ft=ft, player=player, dice=dice)


def first_rolls(n, seed, env0):
    """The roll each of the ids env0 .. env0 + n - 1 sees at ply counter 0
    under the device's dice stream of `seed`, from the oracle: (n, 2) uint8.
    It depends on the seed, the id and the counter, not on the position."""
    import oracle as O

    sp = O.SelfPlay(n, seed, env0)
    sp.reset(0)
    return sp.run(1)["dice"][0].copy()


def place_for_rolls(st, first):
    """A turn_states(n, seed) set permuted for ids that draw their own dice
    (the one-launch rollouts and the playouts): the run-heavy half, in its
    order, goes first to the ids that roll a double -- `first` is the ids'
    (n, 2) first rolls, or (n, trials, 2) where an id is a playout root of
    several trials: one double among them is enough -- in ascending order, and
    every other position, in the set's order, to the ids left.  Returns the
    dict of turn_states(), the dice column the ids' own (trial 0's)."""
    first = np.asarray(first, np.uint8)
    n = len(st["player"])
    rolls = first.reshape(n, -1, 2)
    dbl = (rolls[:, :, 0] == rolls[:, :, 1]).any(1)
    ids = np.concatenate([np.flatnonzero(dbl), np.flatnonzero(~dbl)])
    src = np.empty(n, np.int64)
    src[ids] = np.arange(n)  # position k of the set sits at id ids[k]
    out = {k: np.ascontiguousarray(np.asarray(st[k])[src]) for k in ("board", "off", "ft", "player")}
    out["dice"] = np.ascontiguousarray(rolls[:, 0])
    out["heavy"] = src < n // 2  # which ids hold a position of the run-heavy half
    return out


def spread_replier_states(n, seed):
    """turn_states(n, seed) with the run-heavy half's mover flipped and that
    half's dice never a double: the piled side moves -- few first-ply rows --
    and the spread side replies, whose doubles outgrow the lookahead's fast
    frontier (with the piled side replying no reply walk does)."""
    s = turn_states(n, seed)
    h = n // 2
    s["player"][:h] = -s["player"][:h]
    d = s["dice"][:h]
    same = d[:, 0] == d[:, 1]
    d[same, 1] = d[same, 0] % 6 + 1
    return s
