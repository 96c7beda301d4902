"""The optimiser tests' reference: the norm clip, the
SGD step and AdamW (maximising: theta moves along the gradient) restated in
numpy, explicit formulas, any float dtype.  The tests run it in float64 (the
reference) and in float32 (its own rounding, E of td_ref's rule).

Every hyperparameter enters as the float32 value the C call receives --
float64(float32(0.999)), not 0.999 --: otherwise E would be the rounding of
0.999 itself.  A gradient / moment row is laid out as narde.h states: T[c * H +
h] for column c < 198, then b1's H, w2's H, b2's one.
"""
import numpy as np


def h(x):
    """A hyperparameter as the call receives it: the float32 value, as a float."""
    return float(np.float32(x))


def clip(grad, max_norm, dtype):
    """(norm, coefficient): torch.nn.utils.clip_grad_norm_'s, in dtype."""
    dt = np.dtype(dtype).type
    g = np.asarray(grad, dtype)
    norm = np.sqrt((g * g).sum(dtype=dtype))
    coef = dt(h(max_norm)) / (norm + dt(h(1e-6)))
    return norm, min(dt(1), coef)


def sgd(theta, grad, alpha, dtype, scale=None):
    """theta + alpha (scale grad)."""
    dt = np.dtype(dtype).type
    g = np.asarray(grad, dtype)
    if scale is not None:
        g = dt(scale) * g
    return np.asarray(theta, dtype) + dt(h(alpha)) * g


class Adam:
    """torch.optim.AdamW(maximize=True) on one row, in dtype; weight_decay = 0
    is torch.optim.Adam(maximize=True)."""

    def __init__(self, theta, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, dtype=np.float64):
        self.dt = np.dtype(dtype).type
        self.lr, self.b1, self.b2, self.eps, self.wd = (self.dt(h(x)) for x in (lr, betas[0], betas[1], eps, weight_decay))
        self.theta = np.array(theta, dtype)
        self.m, self.s, self.t = np.zeros_like(self.theta), np.zeros_like(self.theta), 0

    def step(self, grad, scale=None):
        dt, one = self.dt, self.dt(1)
        g = np.asarray(grad, self.theta.dtype)
        if scale is not None:
            g = dt(scale) * g
        self.t += 1
        self.theta = self.theta * (one - self.lr * self.wd)
        self.m = self.b1 * self.m + (one - self.b1) * g
        self.s = self.b2 * self.s + (one - self.b2) * g * g
        bc1, bc2 = one - dt(self.b1 ** dt(self.t)), one - dt(self.b2 ** dt(self.t))
        self.theta = self.theta + (self.lr / bc1) * self.m / (np.sqrt(self.s) / np.sqrt(bc2) + self.eps)
        return self.theta


def synthetic_grads(rows, steps, seed, zero_every, zero_step):
    """(steps, rows) float32: magnitudes 10^-6 .. 10^2 (log-uniform), random
    signs, every zero_every-th element zero, step zero_step all zero."""
    rng = np.random.default_rng(seed)
    g = (10.0 ** rng.uniform(-6, 2, (steps, rows)) * rng.choice([-1.0, 1.0], (steps, rows))).astype(np.float32)
    g[:, ::zero_every] = 0.0
    g[zero_step] = 0.0
    return g
