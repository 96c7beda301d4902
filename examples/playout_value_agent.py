#!/usr/bin/env python3
"""Is a value net calibrated?  Its v(s) against Monte-Carlo playouts of s.

A window of value-greedy self-play is played in one launch with the records
of its positions (VecNardeEnv.value_rollout, --rules full4:
turn_value_rollout; through td.WindowTDLambdaLearner with step size 0, which
also leaves the net's v(s) of every recorded position and changes no weight).
A sample of those positions is then played out to the end, `--trials` times
each, both colours value-greedy under the same net (VecNardeEnv.playout: one
launch, a wave a trial, each trial on its own dice), and the playout mean of
white's points -- what the position turned out to be worth under that policy
-- is set against v(s): mean absolute error and bias over the sample.  A net
whose output is a win probability (sigmoid) is compared after 2 v - 1.  The
fixed-seed 198 -> 80 -> 1 net is untrained: load one with --weights (such as
examples/train_value_agent.py saves).

  python examples/playout_value_agent.py [--envs B] [--plies K] [--sample N] [--trials T] [--max-plies P] [--seed S]
      [--weights FILE] [--rules ref2|full4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def main(envs=256, plies=32, sample=256, trials=32, max_plies=400, seed=0, weights=None, device="cuda", rules="ref2"):
    import torch

    from gym_narde.td import WindowTDLambdaLearner
    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device=device, seed=seed, rules=rules)
    torch.manual_seed(seed)
    net = ValueMLP(80, "sigmoid", "sigmoid")
    if weights:
        sd = torch.load(weights, map_location="cpu")
        if "0.weight" in sd:  # examples/play_value_agent.py's Sequential: the same two layers
            sd = {k.replace("0.", "l1.").replace("2.", "l2."): v for k, v in sd.items()}
        net = ValueMLP(sd["l1.weight"].shape[0], "sigmoid", "sigmoid")
        net.load_state_dict(sd)
    net = net.to(env.device)
    net.pack()

    window = WindowTDLambdaLearner(env, net, alpha=0.0, lam=0.0, plies=plies, seed=seed)
    window.step()  # the window and, with step size 0, v(s) of its positions under the unchanged weights
    records = window.bufs["records"].reshape(-1, 8)
    v = window.values()[:plies].reshape(-1)
    pick = torch.linspace(0, records.shape[0] - 1, min(sample, records.shape[0]), device=env.device).long()
    roots, v = records[pick].contiguous(), v[pick].double()

    res = env.playout(roots, trials, net, max_plies=max_plies, seed=seed + 1)
    torch.cuda.synchronize()
    unfinished = roots.shape[0] * trials - int(res.finished.sum())
    if unfinished:
        raise SystemExit(f"{unfinished} trials did not finish in {max_plies} plies: raise --max-plies")
    mean = res.mean()
    if net.out_act == "sigmoid":  # a probability that white wins -> expected points, gammons aside
        v = 2.0 * v - 1.0
    err = v - mean
    print(f"{roots.shape[0]} positions of a {plies}-ply window of {envs} envs ({rules}), {trials} playouts each: "
          f"{int(res.plies.sum())} plies played, {float(res.plies.sum()) / (roots.shape[0] * trials):.1f} a playout")
    print(f"white's points: playout mean {float(mean.mean()):+.4f} (standard error of a position's mean "
          f"{float(res.stderr().nanmean()):.4f}); v(s) {float(v.mean()):+.4f}")
    print(f"v(s) against the playout mean: mean absolute error {float(err.abs().mean()):.4f}, bias "
          f"{float(err.mean()):+.4f}")
    env.close()
    return float(err.abs().mean()), float(err.mean())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--plies", type=int, default=32)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--trials", type=int, default=32)
    ap.add_argument("--max-plies", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    a = ap.parse_args()
    main(a.envs, a.plies, a.sample, a.trials, a.max_plies, a.seed, a.weights, rules=a.rules)
