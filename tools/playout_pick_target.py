#!/usr/bin/env python3
"""Playout-greedy play's measurement target.

Profiler off, device events.  One 198 -> H -> 1 net (sigmoid, sigmoid; seed 0).

--mode ply: one PlayoutPlayer ply less its step() -- recorded afterstates,
top_rows, playout, pick_playout -- for B envs at the positions they hold after
`--window-plies` plies of value-greedy self-play, against the best the calls
before it offer for the same ply:
  baseline -- scored afterstates for the values and a second expansion with
              obs=True for the boards (cap given: neither synchronises), the
              rows' widest env read on the host, each env's k best rows by a
              padded stable torch.sort, their boards, off counts, flags and
              movers rebuilt in torch from obs, state_records(), the same
              playout(), the means reduced with torch and scattered into a
              row-value tensor for pick_afterstate() / pick_turn().
One warm-up, `--reps` timed runs of each, alternating; ms, min / median / max,
and the new chain's four calls timed one by one.  The two must have the same
candidates and scores; the rows played may differ where two scores tie.

--mode strength: B games a colour assignment of PlayoutPlayer(k, trials)
against value-greedy play under one net trained for `--train-plies` plies of
windowed TD(lambda) self-play (tanh output): PlayoutPlayer's five calls with
the other colour's envs taking pick_afterstate()'s move instead; the playout
side's points a game (negative: lost) and their standard error over the
finished games.

  python tools/playout_pick_target.py [--mode ply|strength] [--rules ref2|full4] [--envs B] [--k K] [--trials T]
      [--max-plies P] [--hidden H] [--reps R] [--window-plies W] [--train-plies N] [--game-plies G]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def span_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4), max=round(max(xs), 4))


def ply_mode(a, torch, VecNardeEnv, ValueMLP):
    full = a.rules == "full4"
    B, k, T = a.envs, a.k, a.trials
    env = VecNardeEnv(B, device="cuda", seed=0, rules=a.rules)
    dev = env.device
    torch.manual_seed(0)
    net = ValueMLP(a.hidden, "sigmoid", "sigmoid").to(dev)
    net.pack()
    W = a.window_plies
    if full:
        off = dict(dice=False, play=False, value=False, reward=False, terminated=False, truncated=False)
        env.turn_value_rollout(W, net, bufs=env.turn_value_rollout_buffers(W, **off))
    else:
        off = dict(dice=False, actions=False, value=False, reward=False, terminated=False, truncated=False)
        env.value_rollout(W, net, bufs=env.value_rollout_buffers(W, **off))
    dice = env.dice().clone()
    recorded = env.recorded_turn_afterstates if full else env.recorded_afterstates
    scored = env.scored_turn_afterstates if full else env.scored_afterstates
    expand = env.turn_afterstates if full else env.afterstates
    pick = env.pick_turn if full else env.pick_afterstate
    probe, _, _ = recorded(None, dice)
    cap = probe.cap
    rows = probe.offsets[1:] - probe.offsets[:-1]
    res = dict(mode="ply", rules=a.rules, envs=B, k=k, trials=T, max_plies=a.max_plies, hidden=a.hidden, reps=a.reps,
               rows=cap, rows_per_env=round(cap / B, 2), widest_env=int(rows.max()))
    kw = dict(max_plies=a.max_plies, seed=1, common_dice=True)
    parts = {n: [] for n in ("records", "top_rows", "playout", "pick")}

    def chain(timed=False):
        t = (lambda f: span_ms(torch, f)) if timed else (lambda f: (0.0, f()))
        ms, (aft, values, records) = t(lambda: recorded(net, dice, cap=cap))
        parts["records"].append(ms)
        ms, (sel, roots) = t(lambda: env.top_rows(aft, values, k, records))
        parts["top_rows"].append(ms)
        ms, out = t(lambda: env.playout(roots, T, net, **kw))
        parts["playout"].append(ms)
        ms, (actions, row, score) = t(lambda: env.pick_playout(aft, values, sel, out))
        parts["pick"].append(ms)
        return row, out, sel, score

    st = env.get_state()
    ft, mover = st["first_turn"], st["player"]
    t_next = env.ply + 1  # the ply counter the step leaves: the playouts' dice start there

    def baseline():
        aft, values = scored(net, dice, cap=cap)
        obs = expand(dice, cap=cap, feat=False, obs=True).obs
        offs = aft.offsets.long()
        cnt = offs[1:] - offs[:-1]
        width = int(cnt.max())  # a synchronise
        idx = offs[:-1, None] + torch.arange(width, device=dev)[None]
        valid = torch.arange(width, device=dev)[None] < cnt[:, None]
        v = values[idx.clamp(max=cap - 1)]
        x = torch.where((mover == -1)[:, None], -v, v)
        key = torch.where(valid, -x, torch.full_like(x, float("inf")))
        order = torch.sort(key, dim=1, stable=True).indices[:, :k]
        if order.shape[1] < k:
            order = torch.cat([order, order.new_zeros(B, k - order.shape[1])], 1)
        has = torch.arange(k, device=dev)[None] < cnt[:, None]
        sel = torch.where(has, offs[:-1, None] + order, torch.zeros_like(order)).reshape(-1)
        # the rows' positions from obs (the board as the player to move sees it), the reward and the parent
        parent = aft.row_env.long()[sel]
        term = aft.reward[sel] != 0
        player = torch.where(term, mover[parent], -mover[parent]).to(torch.int8)
        o = obs[sel]
        board = torch.where((player == 1)[:, None], o, -torch.roll(o, 12, dims=1)).to(torch.int8)
        offw = 15 - board.clamp(min=0).sum(1)
        offb = 15 + board.clamp(max=0).sum(1)
        off_ = torch.stack([offw, offb], 1).to(torch.uint8)
        f = ft[parent].clone()
        white_moved = mover[parent] == 1
        f[:, 0] = torch.where(white_moved, torch.zeros_like(f[:, 0]), f[:, 0])
        f[:, 1] = torch.where(white_moved, f[:, 1], torch.zeros_like(f[:, 1]))
        roots = env.state_records(board, off_, f, player, t=t_next)
        out = env.playout(roots, T, net, **kw)
        mean = (out.points.double() / out.finished.double()).float()
        sc = torch.where(out.finished > 0, mean, values[sel])
        sc = torch.where(term, values[sel], sc)
        worst = torch.where(mover == -1, float("inf"), -float("inf")).float()
        rowv = worst[aft.row_env.long()].clone()
        live = has.reshape(-1)
        rowv[sel[live]] = sc[live]
        _, row = pick(aft, rowv, "white")
        return row, out, torch.where(has, sel.reshape(B, k), -1), sc.reshape(B, k)

    row_new, out_new, sel_new, score_new = chain()
    row_old, out_old, sel_old, score_old = baseline()
    torch.cuda.synchronize()
    # the same candidates with the same scores; the rows played differ only where two candidates' scores tie
    # (the chain takes the better one-ply value, the baseline's pick the lower row)
    live = sel_new >= 0
    res["same_candidates"] = bool(torch.equal(sel_new.long(), sel_old))
    res["same_scores"] = bool(torch.equal(score_new[live], score_old[live]))
    differ = (row_new != row_old).nonzero().reshape(-1)
    slot = lambda row: (sel_new.long() == row.long()[:, None]).float().argmax(1)  # noqa: E731
    e = differ
    tie = score_new[e, slot(row_new)[e]] == score_new[e, slot(row_old)[e]]
    res["rows_differ"] = int(differ.numel())
    res["rows_differ_not_tied"] = int((~tie).sum())
    res["playout_plies"] = int(out_new.plies.sum())
    res["baseline_playout_plies"] = int(out_old.plies.sum())
    for p in parts.values():
        p.clear()
    tn, tb = [], []
    for _ in range(a.reps):  # alternating
        tn.append(span_ms(torch, chain)[0])
        tb.append(span_ms(torch, baseline)[0])
    for p in parts.values():
        p.clear()
    for _ in range(a.reps):
        chain(timed=True)
    res["chain_ms"] = spread(tn)
    res["baseline_ms"] = spread(tb)
    res["ratio_of_medians"] = round(statistics.median(tb) / statistics.median(tn), 4)
    res["parts_ms"] = {n: spread(p) for n, p in parts.items()}
    print(json.dumps(res))
    env.close()


def strength_mode(a, torch, VecNardeEnv, ValueMLP):
    from gym_narde.td import WindowTDLambdaLearner
    B = a.envs
    tr = VecNardeEnv(1024, device="cuda", seed=0, rules=a.rules)
    torch.manual_seed(0)
    net = ValueMLP(a.hidden, "sigmoid", "tanh").to(tr.device)
    learner = WindowTDLambdaLearner(tr, net, alpha=1e-4, lam=0.7, plies=16, epsilon=0.1, seed=0)
    for _ in range(-(-a.train_plies // 16)):
        learner.step()
    net.pack()
    tr.close()
    res = dict(mode="strength", rules=a.rules, games=B, k=a.k, trials=a.trials, max_plies=a.max_plies, hidden=a.hidden,
               train_plies=a.train_plies, game_plies=a.game_plies)
    sides = {}
    for name, playout_colour in (("playout_white", 1), ("playout_black", -1)):
        # one game an env (auto-reset off).  The first mover is drawn per env, so both colours move at every
        # ply: both players' moves are worked out for every env and each env plays its mover's.
        env = VecNardeEnv(B, device="cuda", seed=5, rules=a.rules, autoreset=False)
        recorded = env.recorded_turn_afterstates if env.full else env.recorded_afterstates
        pick = env.pick_turn if env.full else env.pick_afterstate
        done = torch.zeros(B, dtype=torch.bool, device=env.device)
        pts = torch.zeros(B, dtype=torch.float64, device=env.device)  # the playout side's points, negative: lost
        for ply in range(a.game_plies):
            mover = env.get_state()["player"]
            dice = env.dice()
            aft, values, records = recorded(net, dice)
            sel, roots = env.top_rows(aft, values, a.k, records)
            out = env.playout(roots, a.trials, net, max_plies=a.max_plies, seed=7 + ply, common_dice=True)
            a_pp, _, _ = env.pick_playout(aft, values, sel, out)
            a_vp, _ = pick(aft, values, "white")
            ours = mover == playout_colour
            actions = torch.where(ours.reshape((B,) + (1,) * (a_pp.dim() - 1)), a_pp, a_vp)
            _, rew, term, _, _ = env.step(actions)
            new = (term != 0) & ~done
            pts += torch.where(new, rew.double() * torch.where(ours, 1.0, -1.0), torch.zeros_like(pts))
            done |= new
            if bool(done.all()):
                break
        n = int(done.sum())
        p = pts[done]
        sides[name] = dict(finished=n, points_playout=float(p.clamp(min=0).sum()),
                           points_value=float((-p).clamp(min=0).sum()), mean=float(p.mean()),
                           stderr=float(p.std() / n ** 0.5), plies=ply + 1)
        env.close()
    res["by_colour"] = sides
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("ply", "strength"), default="ply")
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--max-plies", type=int, default=400)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-plies", type=int, default=64)
    ap.add_argument("--train-plies", type=int, default=2048)
    ap.add_argument("--game-plies", type=int, default=400)
    a = ap.parse_args()
    import torch

    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    assert torch.cuda.is_available(), "playout_pick_target.py needs a GPU"
    (ply_mode if a.mode == "ply" else strength_mode)(a, torch, VecNardeEnv, ValueMLP)


if __name__ == "__main__":
    main()
