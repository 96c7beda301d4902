"""value_play.league_pairs / league_result / play_league's argument errors:
host arithmetic only (no device)."""
import math

import numpy as np
import pytest
import torch

from gym_narde.value_net import ValueMLP
from gym_narde.value_play import league_pairs, league_result, play_league


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
def test_league_pairs_counts_order_and_no_duplicates(n):
    plain = league_pairs(n)
    assert len(plain) == n * (n - 1)
    assert plain == [(w, b) for w in range(n) for b in range(n) if w != b]
    rnd = league_pairs(n, random=True)
    assert len(rnd) == n * (n - 1) + 2 * n
    who = list(range(n)) + [-1]
    assert rnd == [(w, b) for w in who for b in who if w != b]
    both = league_pairs(n, random=True, self_play=True)
    assert len(both) == n * (n - 1) + 2 * n + n
    assert both == [(w, b) for w in who for b in who if w != b or w >= 0]
    assert (-1, -1) not in both and all((i, i) in both for i in range(n))
    own = league_pairs(n, self_play=True)
    assert len(own) == n * (n - 1) + n and own == [(w, b) for w in range(n) for b in range(n)]
    for pairs in (plain, rnd, both, own):
        assert len(set(pairs)) == len(pairs)


def test_league_pairs_rejects_no_nets():
    with pytest.raises(ValueError):
        league_pairs(0)


def _brute(stats, white, black, n, random):
    P = n + (1 if random else 0)
    g = [[0] * P for _ in range(P)]
    pw = [[0] * P for _ in range(P)]
    pb = [[0] * P for _ in range(P)]
    for e in range(len(stats)):
        w = white[e] if 0 <= white[e] < n else n
        b = black[e] if 0 <= black[e] < n else n
        g[w][b] += int(stats[e][0])
        pw[w][b] += int(stats[e][1])
        pb[w][b] += int(stats[e][2])
    margin = [[math.nan] * P for _ in range(P)]
    bound = [[math.nan] * P for _ in range(P)]
    for i in range(P):
        for j in range(P):
            games = g[i][j] + g[j][i]
            if games:
                margin[i][j] = (pw[i][j] + pb[j][i] - pb[i][j] - pw[j][i]) / games
                bound[i][j] = 2 / math.sqrt(games)
    score = []
    for i in range(P):
        row = [margin[i][j] for j in range(P) if j != i and g[i][j] + g[j][i]]
        score.append(sum(row) / len(row) if row else math.nan)
    return g, pw, pb, margin, bound, score


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_league_result_equals_a_brute_force_loop():
    n = 3
    pairs = league_pairs(n, random=True, self_play=True)  # 15 pairs
    B = 37  # not a multiple of the pair count
    rng = np.random.default_rng(7)
    white = np.array([pairs[e % len(pairs)][0] for e in range(B)], dtype=np.int32)
    black = np.array([pairs[e % len(pairs)][1] for e in range(B)], dtype=np.int32)
    stats = np.zeros((B, 3), dtype=np.int32)
    stats[:, 0] = rng.integers(0, 6, B)
    stats[:, 1] = rng.integers(0, 2 * stats[:, 0] + 1)
    stats[:, 2] = rng.integers(0, 2 * stats[:, 0] + 1)
    # a pairing with no game at all, in either colour assignment: 1 against 2
    dead = ((white == 1) & (black == 2)) | ((white == 2) & (black == 1))
    assert dead.any()
    stats[dead] = 0
    # another spelling of the random participant
    white[white == -1] = np.where(np.arange((white == -1).sum()) % 2 == 0, -1, n + 4)
    res = league_result(stats, white, black, n, random=True)
    g, pw, pb, margin, bound, score = _brute(stats.tolist(), white.tolist(), black.tolist(), n, True)
    for name, ref in (("games", g), ("points_white", pw), ("points_black", pb)):
        assert res[name].dtype == np.int64 and res[name].shape == (n + 1, n + 1)
        assert np.array_equal(res[name], np.asarray(ref)), name
    assert _same(res["margin"], margin) and _same(res["stderr_bound"], bound) and _same(res["score"], score)
    assert np.isnan(res["margin"][1][2]) and np.isnan(res["margin"][2][1])
    m = res["margin"]
    assert _same(m, -m.T)
    assert (np.diag(m)[:n] == 0).all()  # self-play pooled with itself
    assert np.isnan(m[n][n])  # the random participant never meets itself
    totals = [int(res[k].sum()) for k in ("games", "points_white", "points_black")]
    assert totals == stats.sum(0).tolist()
    assert not np.isnan(res["score"]).any()


def test_league_result_without_random_participant():
    stats = np.array([[2, 3, 0], [1, 0, 2], [4, 1, 1]], dtype=np.int64)
    res = league_result(stats, [0, 1, 0], [1, 0, 1], 2)
    assert res["games"].tolist() == [[0, 6], [1, 0]]
    assert res["points_white"].tolist() == [[0, 4], [0, 0]] and res["points_black"].tolist() == [[0, 1], [2, 0]]
    assert res["margin"][0][1] == (4 + 2 - 1 - 0) / 7 and res["margin"][1][0] == -res["margin"][0][1]
    assert res["stderr_bound"][0][1] == 2 / math.sqrt(7)
    assert res["score"].tolist() == [res["margin"][0][1], res["margin"][1][0]]
    with pytest.raises(ValueError):
        league_result(stats, [0, -1, 0], [1, 0, 1], 2)
    with pytest.raises(ValueError):
        league_result(stats[:, :2], [0, 1, 0], [1, 0, 1], 2)
    with pytest.raises(ValueError):
        league_result(stats, [0, 1], [1, 0, 1], 2)
    lone = league_result(np.zeros((1, 3)), [0], [0], 1)
    assert np.isnan(lone["score"]).all() and np.isnan(lone["margin"]).all()


class _Env:
    """What play_league() reads of an env before it touches the device."""

    def __init__(self, num_envs, device):
        self.num_envs, self.device, self.full, self.torch = num_envs, torch.device(device), False, torch


def test_play_league_argument_errors_that_need_no_device():
    nets = [ValueMLP(2, "tanh", "none") for _ in range(3)]
    with pytest.raises(ValueError, match="64"):
        play_league(_Env(8192, "cpu"), [nets[0]] * 65, 10)
    with pytest.raises(ValueError):
        play_league(_Env(8192, "cpu"), [], 10)
    with pytest.raises(TypeError):
        play_league(_Env(8192, "cpu"), [torch.nn.Linear(198, 1)], 10)
    with pytest.raises(ValueError, match="device"):
        play_league(_Env(8192, "cuda:0"), nets, 10)  # the nets are on the CPU
    with pytest.raises(ValueError, match="pairs"):
        play_league(_Env(5, "cpu"), nets, 10)  # 6 pairs
    with pytest.raises(ValueError, match="pairs"):
        play_league(_Env(11, "cpu"), nets, 10, random=True)  # 12 pairs
    with pytest.raises(ValueError):
        play_league(_Env(8, "cpu"), nets, 10, pairs=[])
