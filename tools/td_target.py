#!/usr/bin/env python3
"""The TD(lambda) learner's measurement target.

  kernels  -- `plies` plies of TDLambdaLearner.step() after a warm-up: run it
              under `rocprofv3 --kernel-trace --stats` (a run of its own) for
              the durations of k_td_trace / k_td_delta / k_td_partial /
              k_td_update.  Prints the bytes each pass moves.
  step     -- profiler off: ms per TDLambdaLearner.step() by device events,
              split into play (ValuePlayer.step) and learn (the trace and
              apply calls), and the same update restated in torch float32
              (tesauro198() rows, batched explicit per-sample gradients,
              baddbmm / einsum) on the same env, learn part alone.

  python tools/td_target.py kernels|step [--envs B] [--hidden H] [--plies N] [--rules ref2|full4]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-narde_amd"))


def pass_bytes(B, H):
    """Bytes each pass has to move: the trace pass reads and writes every
    row; the apply pass reads every row once (and writes one partial row a
    slab, read once more)."""
    P = 200 * H + 1
    slabs = (B + 63) // 64
    return {"trace": 2 * B * P * 4, "partial": B * P * 4 + slabs * P * 4, "update": slabs * P * 4 + 3 * P * 4}


def make(envs, hidden, rules, lam=0.7):
    import torch

    from gym_narde.td import TDLambdaLearner
    from gym_narde.value_net import ValueMLP
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(envs, device="cuda", seed=0, rules=rules)
    torch.manual_seed(0)
    net = ValueMLP(hidden, "sigmoid", "tanh").to(env.device)
    cap = envs * (96 if env.full else 40)
    learner = TDLambdaLearner(env, net, alpha=1e-4, lam=lam, epsilon=0.1, cap=cap)
    env.selfplay(40)
    return env, net, learner


class TorchLearner:
    """The same update in torch float32 ops."""

    def __init__(self, env, net, alpha, lam, gamma=1.0):
        import torch

        self.t, self.env, self.net = torch, env, net
        self.alpha, self.decay, self.gamma = alpha, gamma * lam, gamma
        B, H = env.num_envs, net.hidden
        z = dict(dtype=torch.float32, device=env.device)
        self.tw1 = torch.zeros((B, H, 198), **z)
        self.tb1, self.tw2, self.tb2 = torch.zeros((B, H), **z), torch.zeros((B, H), **z), torch.zeros(B, **z)

    def forward(self, x):
        t, n = self.t, self.net
        a = t.sigmoid(t.addmm(n.l1.bias, x, n.l1.weight.t()))
        return a, t.tanh(a @ n.l2.weight.reshape(-1) + n.l2.bias)

    def trace_pass(self):
        t, n = self.t, self.net
        with t.no_grad():
            x = self.env.tesauro198()
            a, v = self.forward(x)
            go = 1 - v * v
            d = go[:, None] * n.l2.weight.reshape(1, -1) * a * (1 - a)
            self.tw1.baddbmm_(d[:, :, None], x[:, None, :], beta=self.decay)
            self.tb1.mul_(self.decay).add_(d)
            self.tw2.mul_(self.decay).add_(go[:, None] * a)
            self.tb2.mul_(self.decay).add_(go)
            self.v, self.black = v, x[:, 197] > 0.5

    def apply_pass(self, reward, term, trunc):
        t, n = self.t, self.net
        with t.no_grad():
            _, v2 = self.forward(self.env.tesauro198())
            r = reward.to(t.float32)
            target = t.where(term.bool(), t.where(self.black, -r, r), t.where(trunc.bool(), self.v, self.gamma * v2))
            delta = target - self.v
            n.l1.weight.add_(t.einsum("b,bhc->hc", delta, self.tw1), alpha=self.alpha)
            n.l1.bias.add_(delta @ self.tb1, alpha=self.alpha)
            n.l2.weight.add_((delta @ self.tw2).reshape(1, -1), alpha=self.alpha)
            n.l2.bias.add_((delta * self.tb2).sum().reshape(1), alpha=self.alpha)
            keep = (~(term.bool() | trunc.bool())).to(t.float32)
            self.tw1.mul_(keep[:, None, None])
            self.tb1.mul_(keep[:, None])
            self.tw2.mul_(keep[:, None])
            self.tb2.mul_(keep)
            return delta


def timed_plies(torch, learner, player, plies, warmup):
    """ms per ply: (play, learn), by device events around each part."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    marks = []
    for ply in range(warmup + plies):
        e = [ev() for _ in range(4)]
        e[0].record()
        learner.trace_pass()
        e[1].record()
        out = player.step()
        e[2].record()
        learner.apply_pass(out[1], out[2], out[3])
        e[3].record()
        if ply >= warmup:
            marks.append(e)
    torch.cuda.synchronize()
    play = sum(e[1].elapsed_time(e[2]) for e in marks) / plies
    learn = sum(e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3]) for e in marks) / plies
    return play, learn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "step"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--plies", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rules", choices=("ref2", "full4"), default="ref2")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "td_target.py needs a GPU"
    env, net, learner = make(a.envs, a.hidden, a.rules)
    res = dict(mode=a.mode, envs=a.envs, hidden=a.hidden, rules=a.rules, plies=a.plies,
               bytes=pass_bytes(a.envs, a.hidden), learner_bytes=learner.memory_bytes())
    if a.mode == "kernels":
        for _ in range(a.warmup + a.plies):
            learner.step()
        torch.cuda.synchronize()
    else:
        from gym_narde.value_play import ValuePlayer

        player = ValuePlayer(env, net, perspective="white", fused=True, cap=learner.player.cap)
        for rep in range(2):
            play, learn = timed_plies(torch, learner, player, a.plies, a.warmup)
            res[f"kernels_run{rep}"] = dict(play_ms=round(play, 4), learn_ms=round(learn, 4))
        ref = TorchLearner(env, net, learner.alpha, learner.lam)
        for rep in range(2):
            play, learn = timed_plies(torch, ref, player, a.plies, a.warmup)
            res[f"torch_run{rep}"] = dict(play_ms=round(play, 4), learn_ms=round(learn, 4))
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
