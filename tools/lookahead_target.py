#!/usr/bin/env python3
"""The two-ply lookahead's measurement target.

  kernels  -- `reps` calls of VecNardeEnv.lookahead_afterstates() on one
              position set after a warm-up: run it under
              `rocprofv3 --kernel-trace --stats` (a run of its own) for the
              durations of k_aft_fill_rec and k_aft_look.
  step     -- profiler off, device events: ms per ValuePlayer.step() at
              plies 1 and 2, and ms per two-ply valuation by the fused call
              against the same valuation composed from the calls that existed
              before it (a second env of the rows' records, one
              scored_afterstates() per roll, torch segment min / max and the
              mean), on the same positions; two runs each.

  python tools/lookahead_target.py kernels|step [--envs B] [--hidden H] [--reps N] [--warmup W]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def make(envs, hidden):
    import torch

    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device="cuda", seed=0)
    torch.manual_seed(0)
    net = ValueMLP(hidden, "sigmoid", "sigmoid").to(env.device)
    env.selfplay(40)  # into the middle game
    return env, net


class Composed:
    """The two-ply values by composition: the rows' records on a second env,
    scored_afterstates() per roll, the replier's best per row by
    scatter_reduce, the pass for a row with no reply, the mean."""

    def __init__(self, env, net):
        import torch

        self.t, self.env, self.net = torch, env, net

    def values(self, dice):
        from gym_narde.vector import VecNardeEnv

        t, env, net = self.t, self.env, self.net
        aft, v1 = env.scored_afterstates(net, dice)
        R = aft.cap
        st = env.get_state()
        e = aft.row_env.long()
        rows = VecNardeEnv(R, device=env.device, autoreset=False)
        rows.set_state(st["board"][e], st["off"][e], st["first_turn"][e], st["player"][e])
        rows.step(aft.codes, dice[e])
        rec = rows.get_state()
        rec = [rec[k].clone() for k in ("board", "off", "first_turn", "player")]
        black = rec[3] == -1
        zero = t.zeros((R, 2), dtype=t.int16, device=env.device)
        total = t.zeros(R, dtype=t.float64, device=env.device)
        n = 0
        for a in range(1, 7):
            for b in range(1, 7):
                d = t.tensor([[a, b]], dtype=t.uint8, device=env.device).repeat(R, 1)
                rows.set_state(*rec)
                rep, v = rows.scored_afterstates(net, d)
                cnt = rep.offsets[1:] - rep.offsets[:-1]
                idx = rep.row_env.long()
                lo = t.full((R,), float("inf"), device=env.device).scatter_reduce(0, idx, v, "amin")
                hi = t.full((R,), float("-inf"), device=env.device).scatter_reduce(0, idx, v, "amax")
                rows.step(zero, d)
                with t.no_grad():
                    passed = net(rows.tesauro198())
                total += t.where(cnt > 0, t.where(black, lo, hi), passed).double()
                n += 1
        rows.close()
        return aft, t.where(aft.reward != 0, v1, (total / n).float())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "step"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "lookahead_target.py needs a GPU"
    env, net = make(a.envs, a.hidden)
    dice = env.dice()
    aft, values = env.lookahead_afterstates(net, dice)
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, reps=a.reps, rows=aft.cap,
               terminal_rows=int((aft.reward != 0).sum()))
    if a.mode == "kernels":
        for _ in range(a.warmup + a.reps):
            env.lookahead_afterstates(net, dice, cap=aft.cap)
        torch.cuda.synchronize()
    else:
        from gym_narde.value_play import ValuePlayer

        comp = Composed(env, net)
        _, want = comp.values(dice)
        res["fused_minus_composed_max"] = float((values - want).abs().max())
        for rep in range(2):
            res[f"fused_run{rep}"] = timed(torch, lambda: env.lookahead_afterstates(net, dice, cap=aft.cap), a.reps, a.warmup)
            res[f"composed_run{rep}"] = timed(torch, lambda: comp.values(dice), max(2, a.reps // 4), 1)
        st = env.get_state()
        for plies in (1, 2):
            player = ValuePlayer(env, net, plies=plies, cap=a.envs * 40)
            for rep in range(2):
                env.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"])
                res[f"step_plies{plies}_run{rep}"] = timed(torch, player.step, a.reps, a.warmup)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
