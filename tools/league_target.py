#!/usr/bin/env python3
"""The league launches' measurement target.

One process, profiler off, device events, outputs off, 200-ply launches from a
fresh reset each span, the median (min .. max) of `--spans` spans, every
comparison alternating the two sides span by span.  A JSON line a figure,
appended to --out.

  table -- the cost of the table: value_rollout_league() with every env on
           pair (0, 1) against value_rollout(net0, net1), at B = 64, 4,096
           and 65,536, both rule sets.
  buys  -- a 16-net round-robin (240 ordered pairs) in one league launch at
           B = 4,096 and 65,536 against the same games as 240 two-net launches
           over 240 envs of B / 240 envs each, made up front; both rule sets.
  nets  -- the league launch at B = 4,096 and 65,536 with N = 1, 4, 16 and 64
           nets (every ordered pair, (i, i) included, spread over the envs), H
           = 80 and 128; both rule sets.  --same-weights: the N nets are copies
           of one net at N places in memory (the same games as N = 1, N times
           the weights' footprint: the control that separates the two).

198 -> H -> 1 (sigmoid, sigmoid), H = 80 unless said otherwise, torch seed 0.

  python tools/league_target.py table|buys|nets [--out FILE] [--spans S] [--plies N] [--envs B [B ...]] [--same-weights]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))

RULES = ("ref2", "full4")


def make_nets(n, hidden, device, same=False):
    import copy

    import torch

    from gym_narde.value_net import ValueMLP

    torch.manual_seed(0)
    nets = [ValueMLP(hidden, "sigmoid", "sigmoid").to(device) for _ in range(1 if same else n)]
    nets += [copy.deepcopy(nets[0]) for _ in range(n - len(nets))]
    for g in nets:
        g.pack()
    return nets


def span_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), spans=len(xs))


def off_bufs(env, plies):
    off = dict(dice=False, value=False, reward=False, terminated=False, truncated=False)
    off["play" if env.full else "actions"] = False
    return (env.turn_value_rollout_buffers if env.full else env.value_rollout_buffers)(plies, **off)


def alternate(torch, sides, spans, prepare):
    """sides: {name: fn}; every span: prepare(), then the side, the sides in
    turn; one untimed round first."""
    out = {k: [] for k in sides}
    for r in range(spans + 1):
        for name, fn in sides.items():
            prepare(name)
            torch.cuda.synchronize()
            ms = span_ms(torch, fn)
            if r:
                out[name].append(ms)
    return {k: stat(v) for k, v in out.items()}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def mode_table(a, torch, VecNardeEnv):
    for rules in RULES:
        for B in a.envs or (64, 4096, 65536):
            env = VecNardeEnv(B, device="cuda", seed=0, rules=rules)
            nets = make_nets(2, 80, env.device)
            table = env.net_table(nets)
            white = torch.zeros(B, dtype=torch.int32, device=env.device)
            black = torch.ones(B, dtype=torch.int32, device=env.device)
            bufs = off_bufs(env, a.plies)
            league = env.turn_value_rollout_league if env.full else env.value_rollout_league
            two = env.turn_value_rollout if env.full else env.value_rollout
            res = alternate(torch, {"league_ms": lambda: league(a.plies, table, white, black, bufs=bufs),
                                    "two_net_ms": lambda: two(a.plies, nets[0], nets[1], bufs=bufs)},
                            a.spans, lambda _: env.reset())
            games = int(env.stats().sum(0)[0])
            emit(a.out, dict(mode="table", rules=rules, envs=B, plies=a.plies, hidden=80, **res,
                             ratio_of_medians=round(res["league_ms"]["median"] / res["two_net_ms"]["median"], 4),
                             games_in_the_last_launch=games))
            env.close()


def mode_buys(a, torch, VecNardeEnv):
    from gym_narde.value_play import league_pairs

    N = 16
    pairs = league_pairs(N)
    for rules in RULES:
        for B in a.envs or (4096, 65536):
            env = VecNardeEnv(B, device="cuda", seed=0, rules=rules)
            nets = make_nets(N, 80, env.device)
            table = env.net_table(nets)
            idx = torch.arange(B, device=env.device) % len(pairs)
            pw = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=env.device)
            pb = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=env.device)
            white, black = pw[idx].contiguous(), pb[idx].contiguous()
            bufs = off_bufs(env, a.plies)
            league = env.turn_value_rollout_league if env.full else env.value_rollout_league
            # the parent's way: an env a pair, of the envs that pair has in the league launch
            sizes = [len(range(p, B, len(pairs))) for p in range(len(pairs))]
            small = [VecNardeEnv(n, device="cuda", seed=0, env_id_offset=sum(sizes[:p]), rules=rules)
                     for p, n in enumerate(sizes)]
            sbufs = [off_bufs(e, a.plies) for e in small]
            scratch = env.turn_value_rollout_scratch(max(sizes)) if env.full else None

            def two_net_launches():
                for e, (i, j), bf in zip(small, pairs, sbufs):
                    if e.full:
                        e.turn_value_rollout(a.plies, nets[i], nets[j], bufs=bf, scratch=scratch)
                    else:
                        e.value_rollout(a.plies, nets[i], nets[j], bufs=bf)

            def prepare(name):
                if name == "league_ms":
                    env.reset()
                else:
                    for e in small:
                        e.reset()

            res = alternate(torch, {"league_ms": lambda: league(a.plies, table, white, black, bufs=bufs),
                                    "two_net_launches_ms": two_net_launches}, a.spans, prepare)
            emit(a.out, dict(mode="buys", rules=rules, envs=B, plies=a.plies, hidden=80, nets=N, pairs=len(pairs),
                             envs_a_pair=[min(sizes), max(sizes)], **res,
                             two_net_over_league=round(res["two_net_launches_ms"]["median"]
                                                       / res["league_ms"]["median"], 3),
                             games_league=int(env.stats().sum(0)[0]),
                             games_two_net=int(sum(int(e.stats().sum(0)[0]) for e in small))))
            for e in small:
                e.close()
            env.close()


def mode_nets(a, torch, VecNardeEnv):
    for rules in RULES:
        for B in a.envs or (4096, 65536):
            env = VecNardeEnv(B, device="cuda", seed=0, rules=rules)
            bufs = off_bufs(env, a.plies)
            league = env.turn_value_rollout_league if env.full else env.value_rollout_league
            for H in (80, 128):
                for N in (1, 4, 16, 64):
                    nets = make_nets(N, H, env.device, a.same_weights)
                    table = env.net_table(nets)
                    e = torch.arange(B, device=env.device)
                    white = (e % N).to(torch.int32).contiguous()
                    black = ((e // N) % N).to(torch.int32).contiguous()
                    res = alternate(torch, {"league_ms": lambda: league(a.plies, table, white, black, bufs=bufs)},
                                    a.spans, lambda _: env.reset())
                    emit(a.out, dict(mode="nets_same_weights" if a.same_weights else "nets", rules=rules, envs=B,
                                     plies=a.plies, hidden=H, nets=N,
                                     weight_bytes=N * 4 * (200 * H + 1), **res))
            env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("table", "buys", "nets"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--spans", type=int, default=7)
    ap.add_argument("--plies", type=int, default=200)
    ap.add_argument("--envs", type=int, nargs="*", default=None)
    ap.add_argument("--same-weights", action="store_true")
    a = ap.parse_args()
    import torch

    from gym_narde.vector import VecNardeEnv

    assert torch.cuda.is_available(), "league_target.py needs a GPU"
    {"table": mode_table, "buys": mode_buys, "nets": mode_nets}[a.mode](a, torch, VecNardeEnv)


if __name__ == "__main__":
    main()
