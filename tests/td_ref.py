"""The TD(lambda) tests' reference: the value MLP's per-sample gradient and
the TD update restated in torch, explicit formulas, any float dtype.  The
tests run it in float64 (the reference) and in float32 (its own rounding, E).

A gradient / trace row is laid out as narde.h states: T[c * H + h] for
column c < 198, then b1's H, w2's H, b2's one.
"""
import numpy as np
import torch

TOL_FACTOR = 8  # the project's rule (tests/test_value_cpu.py): tol = 8 x E

_ACT = {"none": lambda x: x, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu}


def _slope(name, z, a):
    if name == "none":
        return torch.ones_like(a)
    if name == "sigmoid":
        return a * (1 - a)
    if name == "tanh":
        return 1 - a * a
    return (z > 0).to(a.dtype)


def row_floats(hidden):
    return 200 * hidden + 1


def params_of(net, dtype, device=None):
    """(W1 (H,198), b1 (H,), w2 (H,), b2 ()) of a ValueMLP, as dtype."""
    c = lambda p: p.detach().to(device=device or p.device, dtype=dtype)  # noqa: E731
    return c(net.l1.weight), c(net.l1.bias), c(net.l2.weight).reshape(-1), c(net.l2.bias).reshape(())


def value_and_grad(params, x, hidden_act, out_act):
    """x (n,198) -> v (n,), grad rows (n, 200 H + 1), in x's dtype."""
    w1, b1, w2, b2 = params
    z = x @ w1.t() + b1
    a = _ACT[hidden_act](z)
    y = a @ w2 + b2
    v = _ACT[out_act](y)
    go = _slope(out_act, y, v)
    d = go[:, None] * w2[None, :] * _slope(hidden_act, z, a)
    gw1 = x[:, :, None] * d[:, None, :]  # (n, 198, H): column-major, as the row holds it
    return v, torch.cat([gw1.reshape(x.shape[0], -1), d, go[:, None] * a, go[:, None]], 1)


def td_targets(v, v_next, reward, black, terminated, truncated, gamma):
    """delta (n,): the outcome (reward, negated for black) at a terminal step,
    v itself at a truncated one, gamma v(s') otherwise."""
    outcome = torch.where(black.bool(), -reward.to(v.dtype), reward.to(v.dtype))
    target = torch.where(terminated.bool(), outcome, torch.where(truncated.bool(), v, gamma * v_next))
    return target - v


def theta_row(params):
    """The weights in a trace row's layout, (200 H + 1,)."""
    w1, b1, w2, b2 = params
    return torch.cat([w1.t().reshape(-1), b1, w2, b2.reshape(1)])


def error_bound(x32, x64):
    """E of one compared array: max |fp32 restatement - fp64|, floored at one
    float32 ulp of the array's largest magnitude."""
    x32 = np.asarray(x32, np.float64)
    x64 = np.asarray(x64, np.float64)
    e = float(np.abs(x32 - x64).max()) if x64.size else 0.0
    top = np.float32(np.abs(x64).max()) if x64.size else np.float32(0)
    return max(e, float(np.spacing(top)))


class Bound:
    """max error and E over the chunks of one compared array."""

    def __init__(self, what):
        self.what, self.err, self.e, self.top = what, 0.0, 0.0, 0.0

    def add(self, got, x32, x64):
        x64 = np.asarray(x64, np.float64)
        if not x64.size:
            return
        self.err = max(self.err, float(np.abs(np.asarray(got, np.float64) - x64).max()))
        self.e = max(self.e, float(np.abs(np.asarray(x32, np.float64) - x64).max()))
        self.top = max(self.top, float(np.abs(x64).max()))

    def check(self):
        e = max(self.e, float(np.spacing(np.float32(self.top))))
        print(f"{self.what}: E = {e:.3e}, max error = {self.err:.3e} = {self.err / e:.2f} E")
        assert self.err <= TOL_FACTOR * e, (self.what, self.err, e)
        return self.err / e
