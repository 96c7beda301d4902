#!/usr/bin/env python3
"""Two-ply values of given records: the measurement target.

Profiler off, device events (mode records is also what a kernel trace runs).
One 198 -> H -> 1 net (sigmoid, tanh; seed 0), trained for `--train-plies`
plies by examples/train_value_agent.py --window 8 (0: untrained).

ply      B envs at the positions they hold after `--window-plies` plies of
         value-greedy self-play, then `--plies` plies: at every ply, on the
         same positions and dice, the unpruned two-ply ply less its step --
         lookahead_afterstates() / lookahead_turn_afterstates() and the pick --
         and for each k of --ks the pruned one -- recorded rows, top_rows(k),
         lookahead_records(roots), pick_slots() --, every call with the ply's
         cap given (no synchronise inside a span), alternating, one span each;
         the env then steps with the unpruned pick.  ms a ply, min / median /
         max over the plies, and the share of envs (with a row) in which the
         pruned pick is the unpruned one.
records  lookahead_records() on the first n of a roll's rows' records against
         the full search of B envs that made them: `--reps` spans of each.
curve    LookaheadTargetLearner (plies 8, every --every) against
         WindowTDLambdaLearner (plies 8, lambda 0.7) from one initial net for
         `--budget-ms` of device time each, judged by play_match /
         play_turn_match against the initial net.

  python tools/records_lookahead_target.py ply|records|curve [--rules ref2|full4] [--envs B] [--ks 2,4,8] [--plies P]
      [--n N] [--reps R] [--hidden H] [--window-plies W] [--train-plies T] [--every S] [--alpha A] [--budget-ms M]
"""
import argparse
import copy
import importlib.util
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gym-narde_amd"))


def span_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(xs, nd=3):
    return dict(min=round(min(xs), nd), median=round(statistics.median(xs), nd), max=round(max(xs), nd))


def make_net(a, torch, device):
    from gym_narde.value_net import ValueMLP

    torch.manual_seed(0)
    net = ValueMLP(a.hidden, "sigmoid", "tanh").to(device)
    if a.train_plies:
        spec = importlib.util.spec_from_file_location("train_value_agent",
                                                      os.path.join(HERE, "..", "examples", "train_value_agent.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "agent.pt")
            mod.main(envs=1024, plies=a.train_plies, hidden=a.hidden, rules=a.rules, out=path, device="cuda", window=8)
            net.load_state_dict(torch.load(path, map_location=device))
    net.pack()
    return net


def midgame_env(a, torch, net):
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(a.envs, device="cuda", seed=0, rules=a.rules)
    W = a.window_plies
    if env.full:
        off = dict(dice=False, play=False, value=False, reward=False, terminated=False, truncated=False)
        env.turn_value_rollout(W, net, bufs=env.turn_value_rollout_buffers(W, **off))
    else:
        off = dict(dice=False, actions=False, value=False, reward=False, terminated=False, truncated=False)
        env.value_rollout(W, net, bufs=env.value_rollout_buffers(W, **off))
    return env


def run_ply(a, torch):
    ks = [int(x) for x in a.ks.split(",")]
    net = make_net(a, torch, "cuda")
    env = midgame_env(a, torch, net)
    B = a.envs
    full = env.lookahead_turn_afterstates if env.full else env.lookahead_afterstates
    recorded = env.recorded_turn_afterstates if env.full else env.recorded_afterstates
    expand = env.turn_afterstates if env.full else env.afterstates
    pick = env.pick_turn if env.full else env.pick_afterstate
    t_full, t_k = [], {k: [] for k in ks}
    parts = {k: {n: [] for n in ("records", "top_rows", "lookahead_records", "pick_slots")} for k in ks}
    same, with_row, rows_total = {k: 0 for k in ks}, 0, 0

    def unpruned(dice, cap):
        aft, values = full(net, dice, cap=cap)
        return pick(aft, values, "white")

    def pruned(dice, cap, k, timed=None):
        t = (lambda n, f: f()) if timed is None else (lambda n, f: timed(n, f))
        aft, values, records = t("records", lambda: recorded(net, dice, cap=cap))
        sel, roots = t("top_rows", lambda: env.top_rows(aft, values, k, records))
        two = t("lookahead_records", lambda: env.lookahead_records(roots, net))
        return t("pick_slots", lambda: env.pick_slots(aft, values, sel, two.view(B, k)))[:2]

    for ply in range(a.plies + 1):  # ply 0: the warm-up of every shape
        dice = env.dice().clone()
        cap = expand(dice, feat=False).cap  # (the one synchronise, outside the spans)
        ms, (actions, row) = span_ms(torch, lambda: unpruned(dice, cap))
        if ply:
            t_full.append(ms)
            rows_total += cap
            with_row += int((row >= 0).sum())
        for k in ks:
            ms, (_, row_k) = span_ms(torch, lambda: pruned(dice, cap, k))
            if ply:
                t_k[k].append(ms)
                same[k] += int(((row_k == row) & (row >= 0)).sum())

                def timed(name, fn, k=k):
                    ms, out = span_ms(torch, fn)
                    parts[k][name].append(ms)
                    return out

                if ply <= 5:
                    pruned(dice, cap, k, timed)
        env.step(actions)
    res = dict(rows_per_env=round(rows_total / (a.plies * B), 2), unpruned_ms=spread(t_full), pruned={})
    for k in ks:
        res["pruned"][str(k)] = dict(ms=spread(t_k[k]),
                                     unpruned_over_pruned=round(statistics.median(t_full) / statistics.median(t_k[k]), 3),
                                     same_pick=round(same[k] / max(1, with_row), 4),
                                     parts_ms={n: spread(v) for n, v in parts[k].items()})
    env.close()
    return res


def run_records(a, torch):
    net = make_net(a, torch, "cuda")
    env = midgame_env(a, torch, net)
    full = env.lookahead_turn_afterstates if env.full else env.lookahead_afterstates
    recorded = env.recorded_turn_afterstates if env.full else env.recorded_afterstates
    dice = env.dice().clone()
    aft, _, records = recorded(net, dice)
    cap = aft.cap
    n = min(a.n, cap)
    recs = records[:n].contiguous()
    full(net, dice, cap=cap)
    env.lookahead_records(recs, net)
    t_full, t_rec = [], []
    for _ in range(a.reps):  # alternating
        t_full.append(span_ms(torch, lambda: full(net, dice, cap=cap))[0])
        t_rec.append(span_ms(torch, lambda: env.lookahead_records(recs, net))[0])
    env.close()
    return dict(rows=cap, n=n, full_call_ms=spread(t_full), lookahead_records_ms=spread(t_rec),
                full_us_a_row=round(1e3 * statistics.median(t_full) / cap, 4),
                records_us_a_record=round(1e3 * statistics.median(t_rec) / n, 4))


def run_curve(a, torch):
    from gym_narde import td
    from gym_narde.value_play import play_match, play_turn_match
    from gym_narde.vector import VecNardeEnv

    net0 = make_net(a, torch, "cuda")
    judge = VecNardeEnv(a.games, device="cuda", seed=99, rules=a.rules)
    match = play_turn_match if judge.full else play_match

    def strength(net):
        m = match(judge, net, net0, 400)
        n, pa, pb = max(1, m["games"]), m["points_a"], m["points_b"]
        mean = (pa - pb) / n
        # a game gives +-1 or +-2, so sum x^2 <= 2 (pa + pb): an upper bound of the standard error from the totals
        bound = (max(0.0, 2.0 * (pa + pb) / n - mean * mean) / n) ** 0.5
        return dict(games=m["games"], points_a=pa, points_b=pb, mean=round(mean, 4), stderr_at_most=round(bound, 4))

    out = {}
    makers = {
        "window_td": lambda e, n: td.WindowTDLambdaLearner(e, n, alpha=a.alpha, lam=0.7, plies=8, epsilon=0.1),
        "lookahead_targets": lambda e, n: td.LookaheadTargetLearner(e, n, alpha=a.alpha, plies=8, every=a.every,
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
            ms, _ = span_ms(torch, lambda: [learner.step() for _ in range(8)])
            spent += ms
            steps += 8
        out[name] = dict(steps=steps, device_ms=round(spent, 1), **strength(net))
        e.close()
    judge.close()
    return dict(alpha=a.alpha, budget_ms=a.budget_ms, games=a.games, every=a.every, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("ply", "records", "curve"))
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--plies", type=int, default=20)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--window-plies", type=int, default=40)
    ap.add_argument("--train-plies", type=int, default=0)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--alpha", type=float, default=1e-4)
    ap.add_argument("--budget-ms", type=float, default=4000.0)
    ap.add_argument("--games", type=int, default=4096)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "records_lookahead_target.py needs a GPU"
    run = dict(ply=run_ply, records=run_records, curve=run_curve)[a.mode]
    res = dict(mode=a.mode, rules=a.rules, envs=a.envs, hidden=a.hidden, train_plies=a.train_plies,
               window_plies=a.window_plies)
    res.update(run(a, torch))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
