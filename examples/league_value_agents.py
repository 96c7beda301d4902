#!/usr/bin/env python3
"""Which of these value nets is the strongest, and by how much?  Every FILE is
a 198 -> H -> 1 checkpoint as examples/train_value_agent.py saves it (the
widths may differ); all of them -- and, with --random, the random-legal policy
-- play a whole round-robin, every ordered pair (white, black), in ONE launch
on the GPU: env e plays pair e mod the number of pairs for every game it plays
(gym_narde.value_play.play_league over VecNardeEnv.value_rollout_league, or
turn_value_rollout_league with --rules full4).  Prints
the margin table -- row i against column j: i's points a game over j, both
colour assignments pooled, with the bound 2 / sqrt(games) on its standard
error --, the scores (a row's mean) and the games a pairing.

  python examples/league_value_agents.py FILE [FILE ...] [--random] [--rules ref2|full4] [--envs B] [--plies N] [--seed S] [--out-act none|sigmoid|tanh]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def load_net(path, out_act, device):
    import torch

    from gym_narde.value_net import ValueMLP

    sd = torch.load(path, map_location=device)
    net = ValueMLP(sd["l1.weight"].shape[0], "sigmoid", out_act).to(device)
    net.load_state_dict(sd)
    return net.eval()


def main(files, random=False, rules="ref2", envs=4096, plies=400, seed=0, out_act="tanh", device="cuda"):
    from gym_narde.value_play import play_league
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device=device, seed=seed, rules=rules)
    nets = [load_net(f, out_act, env.device) for f in files]
    res = play_league(env, nets, plies, random=random, seed=seed)
    names = [os.path.basename(f) for f in files] + (["random play"] if random else [])
    P = len(names)
    print(f"{P} participants, {len(res['pairs'])} ordered pairs, {envs} envs x {plies} plies in one launch "
          f"({rules}): {int(res['games'].sum())} games finished")
    print("margin: the row's points a game over the column (+- at most 2 / sqrt(games))")
    for i in range(P):
        cells = "  ".join("      --      " if i == j else f"{res['margin'][i][j]:+.3f}+-{res['stderr_bound'][i][j]:.3f}"
                          for j in range(P))
        print(f"  {i:2d}  {cells}")
    print("scores (mean margin over the opponents met):")
    for i in sorted(range(P), key=lambda i: -res["score"][i] if res["score"][i] == res["score"][i] else 1e9):
        print(f"  {i:2d}  {res['score'][i]:+.3f}  {names[i]}")
    print("games a pairing [white][black]:")
    for i in range(P):
        print(f"  {i:2d}  " + " ".join(f"{int(g):6d}" for g in res["games"][i]))
    env.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+", metavar="FILE")
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--plies", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-act", choices=("none", "sigmoid", "tanh"), default="tanh")
    x = ap.parse_args()
    main(x.files, x.random, x.rules, x.envs, x.plies, x.seed, x.out_act)
