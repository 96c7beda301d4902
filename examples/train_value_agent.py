#!/usr/bin/env python3
"""TD(lambda) self-play on the GPU: trains the 198 -> H -> 1 value network
that examples/play_value_agent.py plays with (TD-Gammon's recipe).  Every ply
of every env: the eligibility traces take the gradient of v(s), both sides
play the afterstate that is best for them (epsilon-greedy), and the weights
move by alpha x sum_e delta_e x trace_e -- gym_narde.td.TDLambdaLearner, all
of it on the device.  The output is tanh by default:
outcomes are +-1 and +-2 (white's points, negative when black wins), which a
sigmoid cannot reach.

--window K trains with gym_narde.td.WindowTDLambdaLearner instead (DESIGN.md
section 21): K plies of self-play in one launch, then one update from the
window with the weights held fixed over it -- truncated TD(lambda), no trace
array; --plies is rounded up to whole windows.  The file written is the same.

--playout-targets TRIALS, next to --window K, trains with
gym_narde.td.PlayoutTargetLearner: every window's
positions -- those of every S-th ply with --every S -- are played out TRIALS
times to the end (--max-plies M plies at most) under the net itself, and the
net is fitted onto the playouts' mean outcomes; with --leaf an unfinished trial
counts at the net's value where it stopped (an M-step truncated-rollout
target).  The file written is the same.

--lookahead-targets, next to --window K, trains with
gym_narde.td.LookaheadTargetLearner: every window's
positions (--every S as above) are valued two plies deep under the net itself
-- the expectation, over the mover's rolls, of the mover's best afterstate --
and the net is fitted onto those values.  The file written is the same.

--optimizer sgd|adam, next to --window K (any of the three learners above),
applies the update through gym_narde.td.ValueSGD / ValueAdam (DESIGN.md section
26) instead of the plain call: the learner makes the summed gradient, the
optimiser steps on it on the device -- --lr is Adam's step size (sgd uses
--alpha), --clip C clips the gradient's norm to C first.  The file written is
the same.

  python examples/train_value_agent.py [--envs B] [--plies N] [--hidden H] [--alpha A] [--lam L] [--epsilon E]
                                       [--rules ref2|full4] [--out-act none|sigmoid|tanh] [--seed S] [--out FILE]
                                       [--window K] [--playout-targets TRIALS [--every S] [--max-plies M] [--leaf]]
                                       [--lookahead-targets [--every S]]
                                       [--optimizer sgd|adam [--lr LR] [--clip C]]

Play the result:  python examples/play_value_agent.py --weights FILE --fused
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def main(envs=1024, plies=2000, hidden=80, alpha=1e-4, lam=0.7, epsilon=0.1, rules="ref2", out_act="tanh", seed=0,
         out="value_agent.pt", device="cuda", report=10, window=0, playout_targets=0, every=1, max_plies=400,
         leaf=False, lookahead_targets=False, optimizer=None, lr=1e-3, clip=None):
    import torch

    from gym_narde.td import (LookaheadTargetLearner, PlayoutTargetLearner, TDLambdaLearner, ValueAdam, ValueSGD,
                              WindowTDLambdaLearner)
    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device=device, seed=seed, rules=rules)
    torch.manual_seed(seed)
    net = ValueMLP(hidden, "sigmoid", out_act).to(env.device)
    if playout_targets and not window:
        raise SystemExit("--playout-targets needs --window K (the plies a step plays and draws its roots from)")
    if lookahead_targets and (not window or playout_targets):
        raise SystemExit("--lookahead-targets needs --window K and excludes --playout-targets")
    if (optimizer or clip is not None) and not window:
        raise SystemExit("--optimizer and --clip need --window K (the online learner applies its update itself)")
    opt = None
    if optimizer == "adam":
        opt = ValueAdam(net, lr, max_grad_norm=clip)
    elif optimizer == "sgd" or clip is not None:
        opt = ValueSGD(net, alpha, max_grad_norm=clip)
    if opt is not None:
        alpha = None  # the optimiser has the step size
    fitted = bool(playout_targets or lookahead_targets)
    if lookahead_targets:
        learner = LookaheadTargetLearner(env, net, alpha=alpha, plies=window, every=every, epsilon=epsilon, seed=seed,
                                         optimizer=opt)
        steps, per = -(-plies // window), window
    elif playout_targets:
        learner = PlayoutTargetLearner(env, net, alpha=alpha, plies=window, trials=playout_targets, every=every,
                                       max_plies=max_plies, leaf=leaf, epsilon=epsilon, seed=seed, optimizer=opt)
        steps, per = -(-plies // window), window
    elif window:
        learner = WindowTDLambdaLearner(env, net, alpha=alpha, lam=lam, plies=window, epsilon=epsilon, seed=seed,
                                        optimizer=opt)
        steps, per = -(-plies // window), window
    else:
        learner = TDLambdaLearner(env, net, alpha=alpha, lam=lam, epsilon=epsilon, seed=seed)
        steps, per = plies, 1
    print(f"{envs} envs, hidden {hidden}, out {out_act}: learner memory {learner.memory_bytes() / 1e6:.1f} MB")
    if opt is not None:
        size = f"lr {lr:g}" if optimizer == "adam" else f"alpha {opt.alpha:g}"
        print(f"optimizer {'adam' if optimizer == 'adam' else 'sgd'}: {size}, clip {clip}, "
              f"{opt.memory_bytes() / 1e3:.1f} kB of state")
    period = max(1, steps // max(1, report))
    err = torch.zeros((), device=env.device)
    for step in range(steps):
        if fitted:  # the root-mean-square error against the playout (two-ply) targets
            loss = learner.step()[0]
            err += (loss[0] / loss[1].clamp(min=1.0)).sqrt().float()
        else:
            err += learner.step()[-1].abs().mean()
        if (step + 1) % period == 0 or step + 1 == steps:
            n = (step % period) + 1
            ep = int(env.stats().sum(0)[0])
            what = "rms error" if fitted else "mean |delta|"
            print(f"ply {(step + 1) * per}: {what} {float(err) / n:.4f}, {ep} games finished")
            err.zero_()
    torch.save(net.state_dict(), out)
    print(f"saved {out}")
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=2000)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--alpha", type=float, default=1e-4)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--out-act", choices=("none", "sigmoid", "tanh"), default="tanh")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="value_agent.pt")
    ap.add_argument("--window", type=int, default=0, help="K > 0: windowed TD(lambda), K plies a launch and update")
    ap.add_argument("--playout-targets", type=int, default=0, metavar="TRIALS",
                    help="TRIALS > 0 (with --window K): fit the net onto playouts of each window's positions")
    ap.add_argument("--every", type=int, default=1, help="playout roots: the positions of every S-th ply of a window")
    ap.add_argument("--max-plies", type=int, default=400, help="a playout trial's length bound")
    ap.add_argument("--leaf", action="store_true", help="count an unfinished trial at the net's value where it stopped")
    ap.add_argument("--lookahead-targets", action="store_true",
                    help="(with --window K): fit the net onto the two-ply values of each window's positions")
    ap.add_argument("--optimizer", choices=("sgd", "adam"), default=None,
                    help="(with --window K): step on the summed gradient with ValueSGD (--alpha) or ValueAdam (--lr)")
    ap.add_argument("--lr", type=float, default=1e-3, help="ValueAdam's step size")
    ap.add_argument("--clip", type=float, default=None, help="clip the gradient's norm to this before the step")
    a = ap.parse_args()
    main(a.envs, a.plies, a.hidden, a.alpha, a.lam, a.epsilon, a.rules, a.out_act, a.seed, a.out, window=a.window,
         playout_targets=a.playout_targets, every=a.every, max_plies=a.max_plies, leaf=a.leaf,
         lookahead_targets=a.lookahead_targets, optimizer=a.optimizer, lr=a.lr, clip=a.clip)
