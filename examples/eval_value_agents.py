#!/usr/bin/env python3
"""Is value net A better than net B, or than random play?  Both are
198 -> H -> 1 checkpoints as examples/train_value_agent.py saves them; every
env plays whole games with A as white and B as black, then with the colours
swapped, each colour assignment one launch on the GPU
(gym_narde.value_play.play_match over VecNardeEnv.value_rollout; DESIGN.md
section 19).  Without --b the opponent is the random-legal policy.
--rules full4: whole turns under the real rules, for nets trained with
train_value_agent.py --rules full4 (play_turn_match over turn_value_rollout;
DESIGN.md section 20).

  python examples/eval_value_agents.py --a FILE [--b FILE] [--envs B] [--plies N] [--seed S] [--out-act none|sigmoid|tanh] [--rules ref2|full4]
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


def main(a, b=None, envs=1024, plies=400, seed=0, out_act="tanh", device="cuda", rules="ref2"):
    from gym_narde.value_play import play_match, play_turn_match
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device=device, seed=seed, rules=rules)
    net_a = load_net(a, out_act, env.device)
    net_b = load_net(b, out_act, env.device) if b else None
    res = (play_turn_match if env.full else play_match)(env, net_a, net_b, plies, seed=seed)
    who = os.path.basename(b) if b else "random play"
    print(f"{os.path.basename(a)} against {who}: {envs} envs x {plies} plies a colour assignment, "
          f"{res['games']} games finished, points a {res['points_a']} / b {res['points_b']}")
    for name, v in res["by_colour"].items():
        print(f"  {name}: {v['games']} games, points a {v['points_a']} / b {v['points_b']}")
    env.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", default=None)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-act", choices=("none", "sigmoid", "tanh"), default="tanh")
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    x = ap.parse_args()
    main(x.a, x.b, x.envs, x.plies, x.seed, x.out_act, rules=x.rules)
