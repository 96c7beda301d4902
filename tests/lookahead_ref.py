"""The two-ply lookahead's reference pipeline, shared
by tests/test_lookahead_cpu.py (the replies from reference_afterstates over
the C oracle) and tests/test_gpu_lookahead.py (the replies from
VecNardeEnv.afterstates on a second env of the rows' records).  Test helper,
not a test.

For every non-terminal row and every roll of the dice mode: the replies' feat
from the existing expansion of the row's position, the CPU twin of the net,
terminal replies set to their outcome, min or max by the replier's colour,
for no replies the value of the position the step with the codes (0, 0)
leaves (nearly always the flipped position; narde.h says when not), the mean
-- once in torch float32 and once in float64.  E = the largest difference
between the two, floored at one float32 ulp of the largest magnitude
compared.
"""
import copy

import numpy as np
import torch

import oracle as O


def rolls_of(dice_mode="all36"):
    """The ordered rolls (a, b), a outer, b inner: 36, or the 30 unequal ones."""
    return [(a, b) for a in range(1, 7) for b in range(1, 7) if dice_mode == "all36" or a != b]


def outcomes(v, reward, player):
    """v with the rows that end the game set to their outcome: reward, negated
    when the row's player -- not flipped after a terminal step: the winner --
    is black.  v: a 1-D torch tensor."""
    r = torch.from_numpy(np.asarray(reward).astype(np.float64)).to(v.dtype)
    won = torch.where(torch.from_numpy(np.asarray(player) == -1), -r, r)
    return torch.where(r != 0, won, v)


def segment_best(v, offsets, black, fallback):
    """Per row: min (black replies) or max (white) of v[offsets[r]:offsets[r + 1]],
    fallback[r] for an empty segment.  v, fallback: 1-D torch tensors."""
    out = fallback.clone().numpy()
    ne = np.diff(offsets) > 0
    if ne.any():  # the non-empty segments' starts delimit them: an empty one holds no element
        starts = np.asarray(offsets[:-1])[ne].astype(np.int64)
        vn = v.numpy()
        out[ne] = np.where(np.asarray(black)[ne], np.minimum.reduceat(vn, starts), np.maximum.reduceat(vn, starts))
    return torch.from_numpy(out)


def two_ply(net, replies, black):
    """replies: per roll a dict offsets (R + 1,), feat (N, 198), reward (N,),
    player (N,) of the R rows' reply rows, and pass_feat (R, 198),
    pass_reward (R,), pass_player (R,): what the step with (0, 0) leaves;
    black (R,) bool: black replies.  Returns (fp64 values (R,), fp32 values
    (R,), per roll m in fp64 (R, rolls))."""
    out = []
    for dt in (torch.float64, torch.float32):
        n = copy.deepcopy(net).to(dt)
        f = lambda x: n(torch.from_numpy(np.ascontiguousarray(x)).to(dt)).reshape(-1)  # noqa: E731
        with torch.no_grad():
            ms = []
            for rep in replies:
                v = outcomes(f(rep["feat"]), rep["reward"], rep["player"]) if len(rep["reward"]) else torch.zeros(0, dtype=dt)
                fallback = outcomes(f(rep["pass_feat"]), rep["pass_reward"], rep["pass_player"])
                ms.append(segment_best(v, rep["offsets"], black, fallback))
            m = torch.stack(ms, 1)
            out.append((m.mean(1), m))
    (v64, m64), (v32, _) = out
    return v64.numpy(), v32.double().numpy(), m64.numpy()


def error_bound(x32, x64):
    """E: max |fp32 pipeline - fp64 pipeline|, floored at one float32 ulp of
    the largest magnitude compared."""
    x32, x64 = np.asarray(x32, np.float64), np.asarray(x64, np.float64)
    e = float(np.abs(x32 - x64).max()) if x64.size else 0.0
    top = np.float32(np.abs(x64).max()) if x64.size else np.float32(0)
    return max(e, float(np.spacing(top)))
