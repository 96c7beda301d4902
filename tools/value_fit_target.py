#!/usr/bin/env python3
"""The supervised fit's measurement target.

  fit     -- profiler off: us per narde_value_fit (ValueFitter.step) over the
             K B records of one K-ply records launch at B envs, the targets
             those records' playout targets (trials 4, 8 plies, leaves); one
             warm-up and `reps` timed calls, each between device events.
  window  -- the yardstick: us per narde_value_td_window
             (WindowTDLambdaLearner.update) on the same launch's records, the
             same way.  --package DIR runs it on another checkout's
             gym-narde_amd (the parent commit's, built there).
  step    -- one PlayoutTargetLearner.step() split into launch, playouts
             (targets()) and fit, ms each, one warm-up and `reps` timed steps.
  curve   -- a learning curve: from one initial net, WindowTDLambdaLearner
             (plies 8, lambda 0.7) against PlayoutTargetLearner for `budget_ms`
             of device time each, each judged by a match against the initial
             net over `games` envs a colour assignment (points a game and an
             upper bound of its standard error, from the totals).

  python tools/value_fit_target.py fit|window|step|curve [--envs B] [--plies K] [--hidden H] [--rules ref2|full4]
         [--reps N] [--trials T] [--every S] [--max-plies M] [--leaf] [--budget-ms MS] [--games G] [--package DIR]
Prints one JSON line.
"""
import argparse
import copy
import json
import os
import sys


def spread(xs, digits=2):
    xs = sorted(xs)
    return dict(min=round(xs[0], digits), median=round(xs[len(xs) // 2], digits), max=round(xs[-1], digits))


def timed(torch, fn, reps, warmup=1):
    """ms of each of `reps` calls of fn after `warmup`, by device events."""
    out = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def setup(a):
    import torch

    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(a.envs, device="cuda", seed=0, rules=a.rules)
    torch.manual_seed(0)
    net = ValueMLP(a.hidden, "sigmoid", "tanh").to(env.device)
    env.selfplay(40)
    return torch, env, net


def run_window(a):
    from gym_narde import td

    torch, env, net = setup(a)
    learner = td.WindowTDLambdaLearner(env, net, alpha=1e-6, lam=0.7, plies=a.plies, epsilon=0.1)
    learner.play()
    us = [1e3 * x for x in timed(torch, learner.update, a.reps)]
    env.close()
    return dict(samples=a.envs * a.plies, update_us=spread(us))


def run_fit(a):
    from gym_narde import td

    torch, env, net = setup(a)
    learner = td.PlayoutTargetLearner(env, net, alpha=1e-6, plies=a.plies, trials=4, max_plies=8, leaf=True, epsilon=0.1)
    learner.play()
    learner.targets()
    us = [1e3 * x for x in timed(torch, learner.update, a.reps)]
    bare = td.ValueFitter(env, net, a.envs * a.plies)  # no weights, no v, the loss: the call's cheapest form is the same kernels
    us_plain = [1e3 * x for x in timed(torch, lambda: bare.step(learner.roots, learner.target, alpha=1e-6), a.reps)]
    env.close()
    return dict(samples=a.envs * a.plies, fit_us=spread(us), fit_no_weights_us=spread(us_plain))


def run_step(a):
    from gym_narde import td

    torch, env, net = setup(a)
    learner = td.PlayoutTargetLearner(env, net, alpha=1e-6, plies=a.plies, trials=a.trials, every=a.every,
                                      max_plies=a.max_plies, leaf=a.leaf, epsilon=0.1)
    parts = {"launch": [], "playouts": [], "fit": []}
    for i in range(1 + a.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        learner.play()
        ev[1].record()
        learner.targets()
        ev[2].record()
        learner.update()
        ev[3].record()
        torch.cuda.synchronize()
        if i:
            for j, k in enumerate(parts):
                parts[k].append(ev[j].elapsed_time(ev[j + 1]))
    res = dict(roots=int(learner.roots.shape[0]), trials=a.trials, every=a.every, max_plies=a.max_plies, leaf=a.leaf,
               playout_plies=int(learner.result.plies.sum()), weight_sum=float(learner.weight.sum()),
               parts_ms={k: spread(v, 4) for k, v in parts.items()}, learner_bytes=learner.memory_bytes())
    env.close()
    return res


def run_curve(a):
    from gym_narde import td
    from gym_narde.value_play import play_match, play_turn_match
    from gym_narde.vector import VecNardeEnv

    torch, env, net0 = setup(a)
    env.close()
    judge = VecNardeEnv(a.games, device="cuda", seed=99, rules=a.rules)
    match = play_turn_match if judge.full else play_match

    def strength(net):
        m = match(judge, net, net0, 400)
        n, pa, pb = max(1, m["games"]), m["points_a"], m["points_b"]
        mean = (pa - pb) / n
        # a game gives +-1 or +-2, so sum x^2 <= 2 (pa + pb): an upper bound of the standard error from the totals
        bound = (max(0.0, 2.0 * (pa + pb) / n - mean * mean) / n) ** 0.5
        return dict(games=m["games"], points_a=pa, points_b=pb, mean=round(mean, 4), stderr_at_most=round(bound, 4),
                    by_colour=m["by_colour"])

    out = {}
    makers = {
        "window_td": lambda e, n: td.WindowTDLambdaLearner(e, n, alpha=a.alpha, lam=0.7, plies=8, epsilon=0.1),
        "playout_targets": lambda e, n: td.PlayoutTargetLearner(e, n, alpha=a.alpha, plies=a.plies, trials=a.trials,
                                                                every=a.every, max_plies=a.max_plies, leaf=a.leaf,
                                                                epsilon=0.1),
    }
    for name, mk in makers.items():
        e = VecNardeEnv(a.envs, device="cuda", seed=0, rules=a.rules)
        net = copy.deepcopy(net0)
        learner = mk(e, net)
        learner.step()
        torch.cuda.synchronize()
        spent, steps = 0.0, 0
        while spent < a.budget_ms:
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            for _ in range(8):
                learner.step()
            y.record()
            torch.cuda.synchronize()
            spent += x.elapsed_time(y)
            steps += 8
        out[name] = dict(steps=steps, device_ms=round(spent, 1), **strength(net))
        e.close()
    judge.close()
    return dict(alpha=a.alpha, budget_ms=a.budget_ms, games=a.games, trials=a.trials, every=a.every,
                max_plies=a.max_plies, leaf=a.leaf, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("fit", "window", "step", "curve"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=16)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--max-plies", type=int, default=400)
    ap.add_argument("--leaf", action="store_true")
    ap.add_argument("--alpha", type=float, default=1e-5)
    ap.add_argument("--budget-ms", type=float, default=2000.0)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--package", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import torch

    assert torch.cuda.is_available(), "value_fit_target.py needs a GPU"
    run = dict(fit=run_fit, window=run_window, step=run_step, curve=run_curve)[a.mode]
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, rules=a.rules, plies=a.plies, reps=a.reps,
               package=os.path.relpath(os.path.abspath(a.package)))
    res.update(run(a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
