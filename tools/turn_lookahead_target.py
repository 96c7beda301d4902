#!/usr/bin/env python3
"""The FULL4 two-ply lookahead's measurement target:
seed 0, 40 plies of FULL4 self-play, a 198 -> H -> 1 sigmoid net.

  kernels  -- `reps` calls of VecNardeEnv.lookahead_turn_afterstates() on one
              position set after a warm-up: run it under
              `rocprofv3 --kernel-trace --stats` (a run of its own) for the
              durations of k_turn_fill_rec, k_turn_overflow_rec, k_turn_look,
              k_turn_look_overflow and k_turn_look_mean.
  step     -- profiler off, device events: ms per two-ply valuation by the
              fused call against the same valuation composed from the calls
              that existed before it (a second FULL4 env of the rows' records,
              one scored_turn_afterstates() per unordered roll, torch segment
              min / max, the pass from the dense net, the weighted mean), on
              the same positions, with the largest difference between the two;
              ms per LookaheadPlayer.step() beside the one-ply ValuePlayer's;
              two runs each.  Where the rows fit the short launch (a row's
              rolls over four waves) the call is also timed with a cap just
              past the threshold, which takes one wave a row.
  stats    -- rows, rolls, and the share of (row, roll) walks that leave the
              256-node fast path (the redo words the call leaves in its
              scratch); with --tiers also the share above 2,048 nodes, from
              the test-only host build of the same walk (slow: small B only).

  python tools/turn_lookahead_target.py kernels|step|stats [--envs B] [--hidden H] [--reps N] [--warmup W]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-narde_amd"))

ROLLS = [(a, b) for a in range(1, 7) for b in range(a, 7)]
SPLIT_ROWS = 3072  # kernels_turn_lookahead.h kTurnLookSplitRows


def make(envs, hidden):
    import torch

    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device="cuda", seed=0, rules="full4")
    torch.manual_seed(0)
    net = ValueMLP(hidden, "sigmoid", "sigmoid").to(env.device)
    env.selfplay(40)  # into the middle game
    return env, net


class Composed:
    """The two-ply values by composition: the rows' records on a second env,
    scored_turn_afterstates() per unordered roll, the replier's best per row
    by scatter_reduce, the pass for a row with no reply, the weighted mean;
    CHUNK rows at a time (a second env's rows are bounded by its 32-bit row
    offsets)."""

    CHUNK = 262144  # rows a second env holds: B x 5,220 must stay below 2^31

    def __init__(self, env, net):
        import torch

        self.t, self.env, self.net = torch, env, net

    def values(self, dice):
        t, env, net = self.t, self.env, self.net
        aft, v1 = env.scored_turn_afterstates(net, dice)
        st = env.get_state()
        two = t.empty(aft.cap, dtype=t.float32, device=env.device)
        for r0 in range(0, aft.cap, self.CHUNK):
            sl = slice(r0, min(r0 + self.CHUNK, aft.cap))
            two[sl] = self.rows_values(st, dice, aft.row_env[sl].long(), aft.play[sl])
        return aft, t.where(aft.reward != 0, v1, two)

    def rows_values(self, st, dice, e, play):
        from gym_narde.vector import VecNardeEnv

        t, env, net = self.t, self.env, self.net
        R = len(e)
        rows = VecNardeEnv(R, device=env.device, autoreset=False, rules="full4")
        rows.set_state(st["board"][e], st["off"][e], st["first_turn"][e], st["player"][e])
        rows.step(play, dice[e])
        rec = rows.get_state()
        rec = [rec[k].clone() for k in ("board", "off", "first_turn", "player")]
        black = rec[3] == -1
        none = t.full((R, 4, 2), -1, dtype=t.int8, device=env.device)
        total = t.zeros(R, dtype=t.float64, device=env.device)
        for a, b in ROLLS:
            d = t.tensor([[a, b]], dtype=t.uint8, device=env.device).repeat(R, 1)
            rows.set_state(*rec)
            rep, v = rows.scored_turn_afterstates(net, d)
            cnt = rep.offsets[1:] - rep.offsets[:-1]
            idx = rep.row_env.long()
            lo = t.full((R,), float("inf"), device=env.device).scatter_reduce(0, idx, v, "amin")
            hi = t.full((R,), float("-inf"), device=env.device).scatter_reduce(0, idx, v, "amax")
            rows.step(none, d)
            with t.no_grad():
                passed = net(rows.tesauro198())
            total += t.where(cnt > 0, t.where(black, lo, hi), passed).double() * (1 if a == b else 2)
        rows.close()
        return (total / 36).float()


def timed(torch, fn, reps, warmup):
    """ms per call (mean, min, max) by device events."""
    ms = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return dict(mean=round(sum(ms) / len(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def wide_out(torch, env, cap):
    """Preallocated rows for `cap` rows (a cap past the rows there are)."""
    from gym_narde.vector import TurnAfterstates

    z = dict(device=env.device)
    out = TurnAfterstates(torch.zeros(env.num_envs + 1, dtype=torch.int32, **z), torch.zeros(cap, dtype=torch.int32, **z),
                          torch.zeros((cap, 4, 2), dtype=torch.int8, **z), None, None,
                          torch.zeros(cap, dtype=torch.int8, **z), cap)
    return out, torch.zeros(cap, dtype=torch.float32, **z)


def redo_share(torch, env, aft, rolls):
    """The share of the live rows' (row, roll) walks the last call marked for
    its overflow pass: the redo words (word 29 of a row's 32) in the scratch."""
    words = env._look_scratch[:128 * aft.cap].view(torch.int32).view(aft.cap, 32)
    live = aft.reward == 0
    redo = words[live][:, 29]
    marked = sum(int(((redo >> k) & 1).sum()) for k in range(21))
    return marked, int(live.sum()) * rolls


def tier_shares(torch, env, aft_rows):
    """(share of walks with a level above 256 nodes, above 2,048, the largest
    level) by the host build of the same walk, a 1-unit net."""
    import ctypes

    import numpy as np

    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_turn_lookahead.so"))
    lib.hc_turn_lookahead.restype = ctypes.c_int64
    s = env.get_state()
    c = lambda x, dt: np.ascontiguousarray(x.cpu().numpy(), dtype=dt)  # noqa: E731
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    board, off, ft = c(s["board"], np.int8), c(s["off"], np.uint8), c(s["first_turn"], np.uint8)
    player, dice = c(s["player"], np.int8), c(env.dice(), np.uint8)
    n, cap = len(player), aft_rows
    w = np.zeros(198, np.float32)
    one = np.zeros(1, np.float32)
    o = dict(offsets=np.zeros(n + 1, np.int32), play=np.zeros((cap, 4, 2), np.int8), reward=np.zeros(cap, np.int8),
             value=np.zeros(cap, np.float32), board=np.zeros((cap, 24), np.int8), off=np.zeros((cap, 2), np.uint8),
             ft=np.zeros((cap, 2), np.uint8), player=np.zeros(cap, np.int8), replies=np.zeros((cap, 21), np.int32),
             front=np.zeros((cap, 21), np.int32), terminal=np.zeros((cap, 21), np.uint8),
             best=np.zeros((cap, 21), np.float32))
    lib.hc_turn_lookahead(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice), ctypes.c_int64(cap), 0, P(w),
                          ctypes.c_int64(1), P(one), P(one), P(one), 1, 0, 0,
                          *(P(o[k]) for k in ("offsets", "play", "reward", "value", "board", "off", "ft", "player",
                                              "replies", "front", "terminal", "best")))
    walks = o["replies"] >= 0
    front = o["front"][walks]
    return float((front > 256).mean()), float((front > 2048).mean()), int(front.max()), int(walks.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "step", "stats"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiers", action="store_true")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "turn_lookahead_target.py needs a GPU"
    env, net = make(a.envs, a.hidden)
    dice = env.dice()
    aft, values = env.lookahead_turn_afterstates(net, dice)
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, reps=a.reps, rows=aft.cap, rolls=len(ROLLS),
               terminal_rows=int((aft.reward != 0).sum()))
    if a.mode == "kernels":
        for _ in range(a.warmup + a.reps):
            env.lookahead_turn_afterstates(net, dice, cap=aft.cap)
        torch.cuda.synchronize()
    elif a.mode == "stats":
        torch.cuda.synchronize()
        res["walks_marked"], res["walks"] = redo_share(torch, env, aft, len(ROLLS))
        if a.tiers:
            res["share_above_256"], res["share_above_2048"], res["max_level"], res["walks_host"] = tier_shares(
                torch, env, aft.cap)
    else:
        from gym_narde.value_play import LookaheadPlayer, ValuePlayer

        comp = Composed(env, net)
        _, want = comp.values(dice)
        res["fused_minus_composed_max"] = float((values - want).abs().max())
        for rep in range(2):
            res[f"fused_run{rep}"] = timed(torch, lambda: env.lookahead_turn_afterstates(net, dice, cap=aft.cap),
                                           a.reps, a.warmup)
            res[f"composed_run{rep}"] = timed(torch, lambda: comp.values(dice), max(2, a.reps // 4), 1)
        if aft.cap <= SPLIT_ROWS:  # the other launch shape on the same rows: the same bits, its own time
            out = wide_out(torch, env, SPLIT_ROWS + 1)
            _, v = env.lookahead_turn_afterstates(net, dice, out=out)
            assert torch.equal(v[:aft.cap].view(torch.int32), values.view(torch.int32))
            for rep in range(2):
                res[f"fused_one_wave_a_row_run{rep}"] = timed(
                    torch, lambda: env.lookahead_turn_afterstates(net, dice, out=out), a.reps, a.warmup)
        st = env.get_state()
        players = dict(one_ply=ValuePlayer(env, net, cap=aft.cap * 2), two_ply=LookaheadPlayer(env, net, cap=aft.cap * 2))
        for name, player in players.items():
            for rep in range(2):
                env.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"])
                res[f"step_{name}_run{rep}"] = timed(torch, player.step, a.reps, a.warmup)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
