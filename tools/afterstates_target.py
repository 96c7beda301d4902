#!/usr/bin/env python3
"""Afterstate expansion at B = 65,536 (MEASUREMENT_LOG
M.25): seed 0, 40 plies of random self-play, device dice, cap from a count
pass.

  launches  warm-up, then --reps launches each of afterstates (k_aft_count +
            k_aft_scan + k_aft_fill), pick_afterstate (k_aft_pick<unsigned int>) and
            tesauro198 (k_tesauro198_rows) on the same env.  Run it under
            `rocprofv3 --kernel-trace --stats` for the kernels' durations; it
            writes the row count and the algorithmic bytes to --json.
  table     the kernels' mean durations from that run's kernel_stats csv
            (--stats) and the bytes (--json) as one markdown table: us,
            achieved TB/s, share of the 8 TB/s HBM roof, k_tesauro198_rows of
            the same trace beside them.
  player    profiler off: ValuePlayer.step() (198 -> 80 -> 1 MLP) per ply by
            device events.

--rules full4 (MEASUREMENT_LOG M.26): the same on a
rules="full4" env -- turn_afterstates (k_turn_count + k_turn_overflow<count>
+ k_aft_scan + k_turn_fill + k_turn_overflow<fill>) and pick_turn
(k_aft_pick<unsigned long>) --, with REF2's afterstates launched on a REF2 env in the same
trace, and the share of envs that take the overflow path (a level of more
than 256 nodes: counted on the CPU by the test-only host build of the same
rule functions, tests/hostcheck, on the env's states and dice).

--scored: launches also runs the scored expansion
(scored_afterstates: k_aft_fill_scored; full4: k_turn_fill_scored +
k_turn_overflow_scored) under the 198 -> 80 -> 1 net, --reps times on the same
env in the same trace, and table lists those kernels beside the plain fills;
player times the fused ValuePlayer (a value_net.ValueMLP of the same weights)
beside the unfused one.

Algorithmic bytes: fill = rows x (792 + 4 + 4 + 1, + 96 with --obs) + B x
(32 + 4) (full4: 8 B of play per row in place of 4 B of codes);
k_tesauro198_rows = B x (32 + 792).
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
# (k_aft_pick is one template: <unsigned int, 0> picks REF2's code pairs,
# <unsigned long, ~0> FULL4's plays)
KERNELS = ("k_aft_count", "k_aft_scan", "k_aft_fill", "k_aft_pick<unsigned int", "k_tesauro198_rows")
KERNELS_FULL4 = ("k_turn_count", "k_turn_overflow<false", "k_aft_scan", "k_turn_fill", "k_turn_overflow<true",
                 "k_aft_pick<unsigned long", "k_aft_count", "k_aft_fill", "k_tesauro198_rows")
KERNELS_SCORED = ("k_aft_fill_scored",)
KERNELS_SCORED_FULL4 = ("k_turn_fill_scored", "k_turn_overflow_scored")
FAST_FRONT = 256  # kernels_turn_afterstates.h kTurnFront


def value_mlp(env):
    """play_value_agent.make_net(0)'s weights as a value_net.ValueMLP."""
    from gym_narde.value_net import ValueMLP
    from play_value_agent import make_net

    return ValueMLP.from_sequential(make_net(0, env.device)).pack()


def setup(a):
    import torch

    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(a.envs, device="cuda:0", seed=0, rules=a.rules)
    env.selfplay(40)
    aft = (env.turn_afterstates if env.full else env.afterstates)(obs=a.obs)  # the count pass sizes it
    torch.cuda.synchronize()
    return torch, env, aft


def overflow_share(env):
    """The share of envs with a level of more than FAST_FRONT nodes, and the
    largest level, by the host build of the rule functions."""
    import ctypes

    import numpy as np

    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_turn_afterstates.so"))
    lib.hc_turn_afterstates.restype = ctypes.c_int64
    s = env.get_state()
    c = lambda x, dt: np.ascontiguousarray(x.cpu().numpy(), dtype=dt)  # noqa: E731
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    board, off, ft = c(s["board"], np.int8), c(s["off"], np.uint8), c(s["first_turn"], np.uint8)
    player, dice = c(s["player"], np.int8), c(env.dice(), np.uint8)
    n = len(player)
    offsets, front, z = np.zeros(n + 1, np.int32), np.zeros(n, np.int32), np.zeros(8, np.int8)
    lib.hc_turn_afterstates(ctypes.c_int64(n), P(board), P(off), P(ft), P(player), P(dice), ctypes.c_int64(0),
                            P(offsets), P(front), P(z), P(z), P(z), P(z), P(z), P(z))
    return float((front > FAST_FRONT).mean()), int(front.max()), offsets


def launches(a):
    torch, env, aft = setup(a)
    B, rows = a.envs, aft.cap
    values = torch.rand(rows, dtype=torch.float32, device=env.device)
    tes = torch.empty((B, 198), dtype=torch.float32, device=env.device)
    ref2 = None
    if env.full:  # REF2's expansion in the same trace
        from gym_narde.vector import VecNardeEnv

        ref2 = VecNardeEnv(B, device="cuda:0", seed=0)
        ref2.selfplay(40)
        aft2 = ref2.afterstates()
    if a.scored:
        net = value_mlp(env)
        out_s = (aft._replace(feat=None, obs=None), torch.empty(rows, dtype=torch.float32, device=env.device))
        scored = env.scored_turn_afterstates if env.full else env.scored_afterstates
    for rep in (a.warm, a.reps):
        for _ in range(rep):
            (env.turn_afterstates if env.full else env.afterstates)(out=aft)
        for _ in range(rep if a.scored else 0):
            scored(net, out=out_s)
        for _ in range(rep):
            (env.pick_turn if env.full else env.pick_afterstate)(aft, values)
        for _ in range(rep if ref2 is not None else 0):
            ref2.afterstates(out=aft2)
        for _ in range(rep):
            env.tesauro198(out=tes)
        torch.cuda.synchronize()
    cnt = (aft.offsets[1:] - aft.offsets[:-1]).float()
    res = dict(envs=B, rows=rows, rows_per_env=rows / B, max_rows=int(cnt.max()), obs=bool(a.obs), rules=a.rules,
               scored=bool(a.scored), scored_bytes=rows * ((8 if env.full else 4) + 4 + 1 + 4) + B * (32 + 4),
               fill_bytes=rows * (792 + (8 if env.full else 4) + 4 + 1 + (96 if a.obs else 0)) + B * (32 + 4),
               tes_bytes=B * (32 + 792))
    if env.full:
        share, front, offsets = overflow_share(env)
        assert (offsets == aft.offsets.cpu().numpy()).all(), "the host build and the kernels disagree"
        res.update(overflow_share=share, max_level=front, ref2_rows=aft2.cap,
                   ref2_fill_bytes=aft2.cap * (792 + 4 + 4 + 1) + B * (32 + 4))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"))


def table(a):
    res = json.load(open(a.json))
    full = res.get("rules") == "full4"
    kernels = KERNELS_FULL4 if full else KERNELS
    if res.get("scored"):
        kernels = kernels + (KERNELS_SCORED_FULL4 if full else KERNELS_SCORED)
    mean = {}
    for r in csv.DictReader(open(a.stats)):
        for k in kernels:
            if k in r["Name"]:
                mean[k] = float(r["AverageNs"]) / 1e3
    nbytes = {"k_aft_fill": res["fill_bytes"], "k_tesauro198_rows": res["tes_bytes"]}
    if full:
        nbytes = {"k_turn_fill": res["fill_bytes"], "k_aft_fill": res["ref2_fill_bytes"], "k_tesauro198_rows": res["tes_bytes"]}
    if res.get("scored"):
        nbytes["k_turn_fill_scored" if full else "k_aft_fill_scored"] = res["scored_bytes"]
    print(f"B = {res['envs']}, {res['rows']} rows ({res['rows_per_env']:.2f} per env, max {res['max_rows']}), "
          f"obs {'on' if res['obs'] else 'off'}" +
          (f", rules full4; {100 * res['overflow_share']:.4f} % of envs on the overflow path (largest level "
           f"{res['max_level']}); REF2 in the same trace: {res['ref2_rows']} rows" if full else "") + "\n")
    if full and "k_turn_fill" in mean and "k_aft_fill" in mean:
        print(f"rows/s of the fill pass: FULL4 {res['rows'] / mean['k_turn_fill'] * 1e6:.3e}, "
              f"REF2 {res['ref2_rows'] / mean['k_aft_fill'] * 1e6:.3e}\n")
    print("| kernel | us | algorithmic MB | TB/s | share of 8 TB/s |")
    print("|---|---|---|---|---|")
    for k in kernels:
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

    def run(p):
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
        return dict(ms_per_ply=s.elapsed_time(e) / a.reps, rows_per_ply=rows / a.reps)

    res = dict(envs=a.envs, plies=a.reps, rules=a.rules, **run(ValuePlayer(env, make_net(0, env.device))))
    if a.scored:  # a fresh env at the same point of the same games
        env.close()
        torch, env, _ = setup(a)
        res["fused"] = run(ValuePlayer(env, value_mlp(env)))
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("launches", "table", "player"))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--obs", action="store_true")
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--scored", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    {"launches": launches, "table": table, "player": player}[a.mode](a)
