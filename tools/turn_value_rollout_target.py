#!/usr/bin/env python3
"""The FULL4 value rollout's measurement target.

  kernels  -- a warm-up, then `reps` launches of
              VecNardeEnv.turn_value_rollout(launch_plies): run it under
              `rocprofv3 --kernel-trace --stats` (a run of its own) for
              k_turn_value_rollout's time.
  ply      -- profiler off, device events: ms per ply of turn_value_rollout()
              in 1-ply, 20-ply and 200-ply launches against the path that
              existed before it, the ValuePlayer.step() FULL4 loop with cap =
              96 B, alternating in the same process: 200 plies after 20, two
              runs each, from the same state.
  tiers    -- no GPU: the host build of the walk
              (tests/hostcheck/build/libhostcheck_turn_value_rollout.so) plays
              the same plies from the same reset and counts those whose walk
              outgrew the 256-node tier and ran again in the slab.

198 -> 80 -> 1 (sigmoid, sigmoid), seed 0.

  python tools/turn_value_rollout_target.py kernels|ply|tiers [--envs B] [--hidden H] [--plies N] [--warmup W] [--launch-plies L] [--reps R]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "gym-narde_amd"))


def make_net(hidden, device):
    import torch

    from gym_narde.value_net import ValueMLP

    torch.manual_seed(0)
    net = ValueMLP(hidden, "sigmoid", "sigmoid").to(device)
    return net


def span_ms(torch, fn):
    """ms of fn() on the device, by events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def tiers(a):
    """The share of plies on the second tier, from the host build."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS

    class NetIn(ctypes.Structure):
        _fields_ = [("w1t", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                    ("ld", ctypes.c_int64), ("hidden", ctypes.c_int32), ("hidden_act", ctypes.c_int32),
                    ("out_act", ctypes.c_int32)]

    hc = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "build", "libhostcheck_turn_value_rollout.so"))
    net = make_net(a.hidden, "cpu")
    c = lambda x: np.ascontiguousarray(x.detach().numpy(), dtype=np.float32)  # noqa: E731
    w1t, b1, w2, b2 = c(net.l1.weight.T), c(net.l1.bias), c(net.l2.weight.reshape(-1)), c(net.l2.bias)
    nin = NetIn(w1t.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data, w1t.shape[1], net.hidden,
                HIDDEN_ACTS[net.hidden_act], OUT_ACTS[net.out_act])
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    plies = a.warmup + a.plies

    def chunk(lo, hi):
        n = hi - lo
        sp = O.SelfPlay(n, seed=0, env0=lo)
        sp.reset(0)
        o = dict(dice=np.zeros((plies, n, 2), np.uint8), play=np.zeros((plies, n, 4, 2), np.int8),
                 value=np.zeros((plies, n), np.float32), reward=np.zeros((plies, n), np.int32),
                 term=np.zeros((plies, n), np.uint8), trunc=np.zeros((plies, n), np.uint8),
                 words=np.zeros((plies, n, 4), np.uint32), rows=np.zeros((plies, n), np.int32),
                 row=np.zeros((plies, n), np.int32), explored=np.zeros((plies, n), np.uint8),
                 tier=np.zeros((plies, n), np.uint8), front=np.zeros((plies, n), np.int32),
                 mdice=np.zeros((plies, n), np.int32))
        t = np.zeros(n, np.uint32)
        hc.hc_turn_value_rollout(ctypes.c_int64(n), P(sp.board), P(sp.off), P(sp.ft), P(sp.player), P(sp.elapsed), P(t),
                                 P(sp.stats), ctypes.c_int64(lo), ctypes.c_uint64(0), 0, 1000, plies, 256,
                                 ctypes.byref(nin), ctypes.byref(nin), 0, ctypes.c_float(0.0), ctypes.c_uint64(0),
                                 ctypes.c_int64(0), *(P(v) for v in o.values()))
        timed = slice(a.warmup, plies)
        return int(o["tier"][timed].sum()), int(o["front"][timed].max()), int(o["rows"][timed].sum())

    step = max(1, (a.envs + 15) // 16)
    with ThreadPoolExecutor(max_workers=16) as ex:
        parts = list(ex.map(lambda lo: chunk(lo, min(lo + step, a.envs)), range(0, a.envs, step)))
    total = a.envs * a.plies
    second = sum(p[0] for p in parts)
    return dict(mode="tiers", envs=a.envs, hidden=a.hidden, plies=a.plies, warmup=a.warmup, env_plies=total,
                second_tier_plies=second, second_tier_share=second / total, largest_level=max(p[1] for p in parts),
                rows_per_ply=sum(p[2] for p in parts) / total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "ply", "tiers"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--plies", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launch-plies", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if a.mode == "tiers":
        print(json.dumps(tiers(a)))
        return
    import torch

    from gym_narde.vector import VecNardeEnv

    assert torch.cuda.is_available(), "turn_value_rollout_target.py needs a GPU"
    env = VecNardeEnv(a.envs, device="cuda", seed=0, rules="full4")
    net = make_net(a.hidden, env.device)
    net.pack()
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, resident_waves=env.turn_value_rollout_waves())
    off = dict(dice=False, play=False, value=False, reward=False, terminated=False, truncated=False)
    scratch = env.turn_value_rollout_scratch()
    res["scratch_bytes"] = scratch.numel()
    if a.mode == "kernels":
        bufs = env.turn_value_rollout_buffers(a.launch_plies, **off)
        env.turn_value_rollout(a.warmup, net, bufs=env.turn_value_rollout_buffers(a.warmup, **off), scratch=scratch)
        for _ in range(a.reps):
            env.turn_value_rollout(a.launch_plies, net, bufs=bufs, scratch=scratch)
        torch.cuda.synchronize()
        res.update(launch_plies=a.launch_plies, reps=a.reps)
    else:
        from gym_narde.value_play import ValuePlayer

        res.update(plies=a.plies, warmup=a.warmup)
        env.turn_value_rollout(a.warmup, net, bufs=env.turn_value_rollout_buffers(a.warmup, **off), scratch=scratch)
        st = env.get_state()
        t0 = env.ply

        def restore():
            env.set_state(st["board"], st["off"], st["first_turn"], st["player"], st["elapsed"])
            env.ply = t0
            torch.cuda.synchronize()

        player = ValuePlayer(env, net, cap=96 * a.envs)
        player.step()  # (its arrays' first allocation, the handle's workspace)

        def loop():
            for _ in range(a.plies):
                player.step()

        per = {}
        for L in (1, 20, 200):
            L = min(L, a.plies)
            bufs = env.turn_value_rollout_buffers(L, **off)

            def launches(L=L, bufs=bufs):
                for _ in range(a.plies // L):
                    env.turn_value_rollout(L, net, bufs=bufs, scratch=scratch)

            per[f"rollout_{L}ply_launches"] = launches
        per["valueplayer_step_loop"] = loop
        runs = {name: [] for name in per}
        for _ in range(2):  # the new call and the loop alternate
            for name, fn in per.items():
                restore()
                runs[name].append(round(span_ms(torch, fn) / a.plies, 5))
        for name, r in runs.items():
            res[name + "_ms_per_ply"] = dict(min=min(r), max=max(r))
        restore()
        env.turn_value_rollout(a.plies, net, bufs=env.turn_value_rollout_buffers(a.plies, **off), scratch=scratch)
        res["games_finished_in_the_200_ply_launch"] = int(env.stats().sum(0)[0])
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
