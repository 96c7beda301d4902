#!/usr/bin/env python3
"""Afterstate expansion at B = 65,536 (MEASUREMENT_LOG
M.25): seed 0, 40 plies of random self-play, device dice, cap from a count
pass.

  launches  warm-up, then --reps launches each of afterstates (k_aft_count +
            k_aft_scan + k_aft_fill), pick_afterstate (k_aft_pick) and
            tesauro198 (k_tesauro198_rows) on the same env.  Run it under
            `rocprofv3 --kernel-trace --stats` for the kernels' durations; it
            writes the row count and the algorithmic bytes to --json.
  table     the kernels' mean durations from that run's kernel_stats csv
            (--stats) and the bytes (--json) as one markdown table: us,
            achieved TB/s, share of the 8 TB/s HBM roof, k_tesauro198_rows of
            the same trace beside them.
  player    profiler off: ValuePlayer.step() (198 -> 80 -> 1 MLP) per ply by
            device events.

Algorithmic bytes: fill = rows x (792 + 4 + 4 + 1, + 96 with --obs) + B x
(32 + 4); k_tesauro198_rows = B x (32 + 792).
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-narde_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

HBM_PEAK = 8.0e12
KERNELS = ("k_aft_count", "k_aft_scan", "k_aft_fill", "k_aft_pick", "k_tesauro198_rows")


def setup(a):
    import torch

    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(a.envs, device="cuda:0", seed=0)
    env.selfplay(40)
    aft = env.afterstates(obs=a.obs)  # the count pass sizes it
    torch.cuda.synchronize()
    return torch, env, aft


def launches(a):
    torch, env, aft = setup(a)
    B, rows = a.envs, aft.cap
    values = torch.rand(rows, dtype=torch.float32, device=env.device)
    tes = torch.empty((B, 198), dtype=torch.float32, device=env.device)
    for rep in (a.warm, a.reps):
        for _ in range(rep):
            env.afterstates(out=aft)
        for _ in range(rep):
            env.pick_afterstate(aft, values)
        for _ in range(rep):
            env.tesauro198(out=tes)
        torch.cuda.synchronize()
    cnt = (aft.offsets[1:] - aft.offsets[:-1]).float()
    res = dict(envs=B, rows=rows, rows_per_env=rows / B, max_rows=int(cnt.max()), obs=bool(a.obs),
               fill_bytes=rows * (792 + 4 + 4 + 1 + (96 if a.obs else 0)) + B * (32 + 4), tes_bytes=B * (32 + 792))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"))


def table(a):
    res = json.load(open(a.json))
    mean = {}
    for r in csv.DictReader(open(a.stats)):
        for k in KERNELS:
            if k in r["Name"]:
                mean[k] = float(r["AverageNs"]) / 1e3
    nbytes = {"k_aft_fill": res["fill_bytes"], "k_tesauro198_rows": res["tes_bytes"]}
    print(f"B = {res['envs']}, {res['rows']} rows ({res['rows_per_env']:.2f} per env, max {res['max_rows']}), "
          f"obs {'on' if res['obs'] else 'off'}\n")
    print("| kernel | us | algorithmic MB | TB/s | share of 8 TB/s |")
    print("|---|---|---|---|---|")
    for k in KERNELS:
        if k not in mean:
            print(f"| {k} | not measured | | | |")
        elif k in nbytes:
            rate = nbytes[k] / (mean[k] * 1e-6)
            print(f"| {k} | {mean[k]:.1f} | {nbytes[k] / 1e6:.1f} | {rate / 1e12:.2f} | {rate / HBM_PEAK:.2f} |")
        else:
            print(f"| {k} | {mean[k]:.1f} | | | |")


def player(a):
    torch, env, _ = setup(a)
    from gym_narde.value_play import ValuePlayer
    from play_value_agent import make_net

    p = ValuePlayer(env, make_net(0, env.device))
    for _ in range(a.warm):
        p.step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rows = 0
    for _ in range(a.reps):
        rows += p.step()[5].cap
    e.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(envs=a.envs, plies=a.reps, ms_per_ply=s.elapsed_time(e) / a.reps,
                          rows_per_ply=rows / a.reps)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("launches", "table", "player"))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--obs", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    {"launches": launches, "table": table, "player": player}[a.mode](a)
