#!/usr/bin/env python3
"""The windowed TD(lambda) learner's measurement target.

  window   -- profiler off: ms per trained ply of WindowTDLambdaLearner.step(),
              (launch + update) / plies by device events, split into the
              records launch and the update; two runs of `windows` windows
              after `warmup`.
  online   -- the baseline: ms per ply of TDLambdaLearner.step() with cap
              given, on the same seed, two runs of windows x plies plies after
              warmup x plies.  --package DIR runs it on another checkout's
              gym-narde_amd (the parent commit's, built there).
  kernels  -- `windows` windows after a warm-up and nothing else: run it under
              `rocprofv3 --kernel-trace --stats` (a run of its own) for the
              per-kernel split.

  python tools/td_window_target.py window|online|kernels [--envs B] [--hidden H] [--plies K] [--rules ref2|full4]
                                                         [--windows N] [--warmup W] [--package DIR]
Prints one JSON line.
"""
import argparse
import json
import os
import sys


def make(mode, envs, hidden, rules, plies, lam=0.7):
    import torch

    from gym_narde import td
    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device="cuda", seed=0, rules=rules)
    torch.manual_seed(0)
    net = ValueMLP(hidden, "sigmoid", "tanh").to(env.device)
    env.selfplay(40)
    if mode == "online":
        cap = envs * (96 if env.full else 40)
        return env, td.TDLambdaLearner(env, net, alpha=1e-4, lam=lam, epsilon=0.1, cap=cap)
    return env, td.WindowTDLambdaLearner(env, net, alpha=1e-4, lam=lam, plies=plies, epsilon=0.1)


def timed_windows(torch, learner, windows, warmup):
    """ms per window: (launch, update), by device events around each part."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    marks = []
    for w in range(warmup + windows):
        e = [ev() for _ in range(3)]
        e[0].record()
        learner.play()
        e[1].record()
        learner.update()
        e[2].record()
        if w >= warmup:
            marks.append(e)
    torch.cuda.synchronize()
    return (sum(e[0].elapsed_time(e[1]) for e in marks) / windows, sum(e[1].elapsed_time(e[2]) for e in marks) / windows)


def timed_steps(torch, learner, steps, warmup):
    """ms per TDLambdaLearner.step(), by device events around the run."""
    for _ in range(warmup):
        learner.step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        learner.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("window", "online", "kernels"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--package", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import torch

    assert torch.cuda.is_available(), "td_window_target.py needs a GPU"
    env, learner = make(a.mode, a.envs, a.hidden, a.rules, a.plies)
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, rules=a.rules, plies=a.plies, windows=a.windows,
               package=os.path.abspath(a.package), learner_bytes=learner.memory_bytes())
    if a.mode == "kernels":
        for _ in range(a.warmup + a.windows):
            learner.step()
        torch.cuda.synchronize()
    elif a.mode == "window":
        for rep in range(2):
            launch, update = timed_windows(torch, learner, a.windows, a.warmup)
            res[f"run{rep}"] = dict(launch_ms_per_ply=round(launch / a.plies, 5), update_ms_per_ply=round(update / a.plies, 5),
                                    ms_per_ply=round((launch + update) / a.plies, 5))
    else:
        for rep in range(2):
            res[f"run{rep}"] = dict(ms_per_ply=round(timed_steps(torch, learner, a.windows * a.plies, a.warmup * a.plies), 5))
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
