#!/usr/bin/env python3
"""The optimiser steps' measurement target.  Profiler
off, device events.

  steps    -- us per narde_value_adam_step, narde_value_sgd_step and
              narde_value_grad_norm alone on a 198 -> H -> 1 net (a span of
              `chain` calls between two events, `reps` spans), against
              torch.optim.Adam(fused=True) over the module's four parameters
              plus the pack() it needs, the same way.
  learner  -- WindowTDLambdaLearner at `plies` plies and B envs: update() alone
              and a whole step(), and ValueFitter.step() on the K B records of
              one launch -- the plain call, ValueSGD and ValueAdam (clip 1), one
              learner each from the same seed, alternating in one loop, `reps`
              rounds after a warm-up.
  curve    -- a learning curve: from one initial net, windowed TD(lambda)
              (plies 8, lambda 0.7, epsilon 0.1) through ValueSGD(alpha) and
              through ValueAdam at each of --lrs, `budget_ms` of device time
              each, judged by a match against the initial net over `games` envs
              a colour assignment.

  python tools/value_optim_target.py steps|learner|curve [--envs B] [--plies K] [--hidden H] [--rules ref2|full4]
         [--reps N] [--chain C] [--alpha A] [--lrs LR,LR,..] [--budget-ms MS] [--games G]
Prints one JSON line.
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def spread(xs, digits=2):
    xs = sorted(xs)
    return dict(min=round(xs[0], digits), median=round(xs[len(xs) // 2], digits), max=round(xs[-1], digits))


def span_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def setup(a):
    import torch

    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(a.envs, device="cuda", seed=0, rules=a.rules)
    torch.manual_seed(0)
    net = ValueMLP(a.hidden, "sigmoid", "tanh").to(env.device)
    env.selfplay(40)
    return torch, env, net


def run_steps(a):
    import torch

    from gym_narde import td
    from gym_narde.value_net import ValueMLP

    torch.manual_seed(0)
    rows = 200 * a.hidden + 1
    grad = torch.randn(rows, device="cuda") * 1e-2

    def chain_us(make):
        """us a call: `reps` spans of `chain` calls after one warm-up span"""
        fn = make()
        out = []
        for i in range(1 + a.reps):
            ms = span_ms(torch, lambda: [fn() for _ in range(a.chain)])
            if i:
                out.append(1e3 * ms / a.chain)
        return spread(out)

    def ours(kind, clip):
        def make():
            net = ValueMLP(a.hidden, "sigmoid", "tanh").to("cuda")
            opt = td.ValueAdam(net, 1e-6, max_grad_norm=clip) if kind == "adam" else td.ValueSGD(net, 1e-6, max_grad_norm=clip)
            return lambda: opt.step(grad)
        return make

    def norm_alone():
        net = ValueMLP(a.hidden, "sigmoid", "tanh").to("cuda")
        opt = td.ValueSGD(net, 0.0, max_grad_norm=1.0)
        return lambda: opt._scale(grad)

    def torch_fused(pack):
        def make():
            net = ValueMLP(a.hidden, "sigmoid", "tanh").to("cuda")
            net.pack()
            opt = torch.optim.Adam(net.parameters(), lr=1e-6, fused=True, maximize=True)
            H = a.hidden
            views = [grad[:198 * H].view(198, H).t().contiguous(), grad[198 * H:199 * H].clone(),
                     grad[199 * H:200 * H].view(1, H).clone(), grad[200 * H:].clone()]
            for p, g in zip(net.parameters(), views):
                p.grad = g

            def step():
                opt.step()
                if pack:
                    net.pack()
            return step
        return make

    return dict(rows=rows, chain=a.chain,
                adam_us=chain_us(ours("adam", None)), sgd_us=chain_us(ours("sgd", None)), norm_us=chain_us(norm_alone),
                adam_clip_us=chain_us(ours("adam", 1.0)), sgd_clip_us=chain_us(ours("sgd", 1.0)),
                torch_fused_adam_us=chain_us(torch_fused(False)), torch_fused_adam_pack_us=chain_us(torch_fused(True)))


def run_learner(a):
    from gym_narde import td
    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    import torch

    def variant(kind):
        env = VecNardeEnv(a.envs, device="cuda", seed=0, rules=a.rules)
        torch.manual_seed(0)
        net = ValueMLP(a.hidden, "sigmoid", "tanh").to(env.device)
        env.selfplay(40)
        opt = {"plain": None, "sgd": td.ValueSGD(net, 1e-6), "adam": td.ValueAdam(net, 1e-6, max_grad_norm=1.0)}[kind]
        alpha = 1e-6 if opt is None else None
        learner = td.WindowTDLambdaLearner(env, net, alpha, lam=0.7, plies=a.plies, epsilon=0.1, optimizer=opt)
        learner.step()
        n = a.envs * a.plies
        fitter = td.ValueFitter(env, net, n, optimizer=opt)
        records = learner.bufs["records"].reshape(n, 8).clone()
        target = torch.zeros(n, device=env.device)
        fit = (lambda: fitter.step(records, target, alpha=1e-6)) if opt is None else (lambda: fitter.step(records, target))
        fit()
        torch.cuda.synchronize()
        return env, learner, fit

    kinds = ("plain", "sgd", "adam")
    made = {k: variant(k) for k in kinds}
    times = {k: dict(update_us=[], step_ms=[], fit_us=[]) for k in kinds}
    for rep in range(a.reps):
        order = kinds if rep % 2 == 0 else kinds[::-1]  # alternating
        for k in order:
            env, learner, fit = made[k]
            times[k]["update_us"].append(1e3 * span_ms(torch, learner.update))
            times[k]["step_ms"].append(span_ms(torch, learner.step))
            times[k]["fit_us"].append(1e3 * span_ms(torch, fit))
    for env, *_ in made.values():
        env.close()
    return dict(samples=a.envs * a.plies,
                **{k: dict(update_us=spread(v["update_us"]), step_ms=spread(v["step_ms"], 3), fit_us=spread(v["fit_us"]))
                   for k, v in times.items()})


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
        return dict(games=m["games"], points_a=pa, points_b=pb, mean=round(mean, 4), stderr_at_most=round(bound, 4))

    makers = {f"sgd_alpha_{a.alpha:g}": lambda n: td.ValueSGD(n, a.alpha)}
    for lr in a.lrs:
        makers[f"adam_lr_{lr:g}"] = lambda n, lr=lr: td.ValueAdam(n, lr)
    out = {}
    for name, mk in makers.items():
        e = VecNardeEnv(a.envs, device="cuda", seed=0, rules=a.rules)
        net = copy.deepcopy(net0)
        learner = td.WindowTDLambdaLearner(e, net, None, lam=0.7, plies=8, epsilon=0.1, optimizer=mk(net))
        learner.step()
        torch.cuda.synchronize()
        spent, steps = 0.0, 0
        while spent < a.budget_ms:
            spent += span_ms(torch, lambda: [learner.step() for _ in range(8)])
            steps += 8
        finite = bool(all(torch.isfinite(p).all() for p in net.parameters()))
        out[name] = dict(steps=steps, device_ms=round(spent, 1), finite=finite, **strength(net))
        e.close()
    judge.close()
    return dict(budget_ms=a.budget_ms, games=a.games, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("steps", "learner", "curve"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--alpha", type=float, default=1e-4)
    ap.add_argument("--lrs", type=lambda s: [float(x) for x in s.split(",")], default=[1e-4, 3e-4, 1e-3])
    ap.add_argument("--budget-ms", type=float, default=4000.0)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "value_optim_target.py needs a GPU"
    run = dict(steps=run_steps, learner=run_learner, curve=run_curve)[a.mode]
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, rules=a.rules, plies=a.plies, reps=a.reps)
    res.update(run(a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
