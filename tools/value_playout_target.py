#!/usr/bin/env python3
"""The playouts' measurement target.

Profiler off, device events.  N roots x `trials` trials, both colours under
one 198 -> H -> 1 net (sigmoid, sigmoid; seed 0), from the start position
(--roots start) or from the positions N envs hold after a `--window-plies`-ply
window of value-greedy self-play (--roots window).

  playout  -- VecNardeEnv.playout(max_plies): ms a launch, ms per played ply
              (the launch's time over sums[:, 3]'s total) and ms per finished
              game;
  baseline -- the best the calls before it offer for the same question: a
              second env of B = N * trials envs set_state()-ed to the roots,
              one value_rollout() / turn_value_rollout() of max_plies plies
              with reward and terminated written (the caller needs them to
              find each env's first terminal ply), max_episode_steps = 0.  Its
              useful plies are the playout's: the plies up to each env's first
              terminal ply.

max_plies: --max-plies, or (default) the longest game of a first, untimed
playout of 1,000 plies plus 10 %.  A warm-up launch, then `--reps` timed
launches of each, alternating; min / median / max.

  python tools/value_playout_target.py [--rules ref2|full4] [--roots start|window] [--n N] [--trials T]
      [--hidden H] [--max-plies P] [--reps R] [--window-plies K]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def span_ms(torch, fn):
    """ms of fn() on the device, by events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(xs):
    return dict(min=round(min(xs), 6), median=round(statistics.median(xs), 6), max=round(max(xs), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--roots", choices=("start", "window"), default="start")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--max-plies", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-plies", type=int, default=64)
    a = ap.parse_args()
    import torch

    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    assert torch.cuda.is_available(), "value_playout_target.py needs a GPU"
    full = a.rules == "full4"
    N, T = a.n, a.trials
    src = VecNardeEnv(N, device="cuda", seed=0, rules=a.rules)
    torch.manual_seed(0)
    net = ValueMLP(a.hidden, "sigmoid", "sigmoid").to(src.device)
    net.pack()
    roll = (lambda e, *x, **k: e.turn_value_rollout(*x, **k)) if full else (lambda e, *x, **k: e.value_rollout(*x, **k))
    buffers = (lambda e, *x, **k: e.turn_value_rollout_buffers(*x, **k)) if full else (
        lambda e, *x, **k: e.value_rollout_buffers(*x, **k))
    column = "play" if full else "actions"
    if a.roots == "window":  # K plies of value-greedy self-play first: middle-game positions, both movers
        K = a.window_plies
        off = dict(dice=False, value=False, reward=False, terminated=False, truncated=False)
        off[column] = False
        roll(src, K, net, bufs=buffers(src, K, **off))
    st = src.get_state()
    if a.roots == "start":
        st["player"] = torch.ones_like(st["player"])
    roots = src.state_records(st["board"], st["off"], st["first_turn"], st["player"])
    res = dict(rules=a.rules, roots=a.roots, n=N, trials=T, hidden=a.hidden, reps=a.reps)

    max_plies = a.max_plies
    if max_plies <= 0:
        probe = src.playout(roots, T, net, max_plies=1000, per_trial=True)
        torch.cuda.synchronize()
        assert int(probe.finished.sum()) == N * T, "a game did not end within 1,000 plies"
        longest = int(probe.length.max())
        max_plies = longest + (longest + 9) // 10
        res["longest_game_plies"] = longest
    res["max_plies"] = max_plies

    out = src.playout(roots, T, net, max_plies=max_plies)  # warm-up; the result's arrays are reused
    torch.cuda.synchronize()
    played, finished = int(out.plies.sum()), int(out.finished.sum())
    res.update(plies_played=played, games_finished=finished)

    # the baseline's env: the roots' positions, each `trials` times over
    base = VecNardeEnv(N * T, device="cuda", seed=0, max_episode_steps=0, rules=a.rules)
    lay = dict(dice=False, value=False, truncated=False)
    lay[column] = False
    bufs = buffers(base, max_plies, **lay)
    state = tuple(st[k].repeat_interleave(T, dim=0) for k in ("board", "off", "first_turn", "player"))

    def baseline():
        base.set_state(*state)
        roll(base, max_plies, net, bufs=bufs)

    baseline()
    torch.cuda.synchronize()
    term = bufs["terminated"].bool()
    done = term.any(0)
    first = torch.where(done, term.int().argmax(0), torch.full_like(done, max_plies - 1, dtype=torch.int64))
    res.update(baseline_useful_plies=int((first + 1).sum()), baseline_plies=max_plies * N * T,
               baseline_games_finished=int(done.sum()))

    tp, tb = [], []
    for _ in range(a.reps):  # alternating
        tp.append(span_ms(torch, lambda: src.playout(roots, T, net, max_plies=max_plies, out=out)))
        tb.append(span_ms(torch, baseline))
    res["playout_ms"] = spread(tp)
    res["baseline_ms"] = spread(tb)
    res["playout_us_per_played_ply"] = spread([1e3 * x / played for x in tp])
    res["playout_ms_per_finished_game"] = spread([x / max(finished, 1) for x in tp])
    res["baseline_us_per_useful_ply"] = spread([1e3 * x / res["baseline_useful_plies"] for x in tb])
    res["baseline_ms_per_finished_game"] = spread([x / max(res["baseline_games_finished"], 1) for x in tb])
    print(json.dumps(res))
    for e in (src, base):
        e.close()


if __name__ == "__main__":
    main()
