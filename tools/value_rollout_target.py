#!/usr/bin/env python3
"""The value rollout's measurement target.

  kernels  -- a warm-up, then `reps` launches of
              VecNardeEnv.value_rollout(launch_plies): run it under
              `rocprofv3 --kernel-trace --stats` (a run of its own) for
              k_value_rollout's time.
  ply      -- profiler off, device events: ms per ply of value_rollout() in
              1-ply, 20-ply and 200-ply launches against the path that
              existed before it, the ValuePlayer.step() loop with cap = 40 B,
              in the same process: 200 plies after 20, two runs each, from the
              same state.

198 -> 80 -> 1 (sigmoid, sigmoid), seed 0.

  python tools/value_rollout_target.py kernels|ply [--envs B] [--hidden H] [--plies N] [--warmup W] [--launch-plies L] [--reps R]
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
    net.pack()
    return env, net


def span_ms(torch, fn):
    """ms of fn() on the device, by events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "ply"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--plies", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launch-plies", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "value_rollout_target.py needs a GPU"
    env, net = make(a.envs, a.hidden)
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden)
    off = dict(dice=False, actions=False, value=False, reward=False, terminated=False, truncated=False)
    if a.mode == "kernels":
        bufs = env.value_rollout_buffers(a.launch_plies, **off)
        env.value_rollout(a.warmup, net, bufs=env.value_rollout_buffers(a.warmup, **off))
        for _ in range(a.reps):
            env.value_rollout(a.launch_plies, net, bufs=bufs)
        torch.cuda.synchronize()
        res.update(launch_plies=a.launch_plies, reps=a.reps)
    else:
        from gym_narde.value_play import ValuePlayer

        res.update(plies=a.plies, warmup=a.warmup)
        env.value_rollout(a.warmup, net, bufs=env.value_rollout_buffers(a.warmup, **off))
        st = env.get_state()
        t0 = env.ply

        def restore():
            env.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"])
            env.ply = t0
            torch.cuda.synchronize()

        player = ValuePlayer(env, net, cap=40 * a.envs)
        player.step()  # (its arrays' first allocation)

        def loop():
            for _ in range(a.plies):
                player.step()

        per = {}
        for L in (1, 20, 200):
            L = min(L, a.plies)
            bufs = env.value_rollout_buffers(L, **off)

            def launches(L=L, bufs=bufs):
                for _ in range(a.plies // L):
                    env.value_rollout(L, net, bufs=bufs)

            per[f"rollout_{L}ply_launches"] = launches
        per["valueplayer_step_loop"] = loop
        for name, fn in per.items():
            runs = []
            for _ in range(2):
                restore()
                runs.append(round(span_ms(torch, fn) / a.plies, 5))
            res[name + "_ms_per_ply"] = dict(min=min(runs), max=max(runs))
        restore()
        env.value_rollout(a.plies, net, bufs=env.value_rollout_buffers(a.plies, **off))
        res["games_finished_in_the_200_ply_launch"] = int(env.stats().sum(0)[0])
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
