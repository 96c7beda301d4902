"""TD(lambda) self-play for a value_net.ValueMLP, on the device (DESIGN.md
section 16): the learner the value-greedy path (value_play.ValuePlayer) was
missing.

Every ply, for all B envs at once:
    trace  <- gamma lam trace + grad_theta v(s)         narde_value_td_trace
    a ply of value-greedy play (epsilon-greedy with epsilon)   ValuePlayer.step
    delta  <- target - v(s),  theta <- theta + alpha sum_e delta_e trace_e
                                                        narde_value_td_apply
with target = the outcome at a terminal step, v(s) at a truncated one (no
successor under autoreset) and gamma v(s') otherwise.  Values are white's
(the README's reward, +1 / +2 if WHITE wins, negated for black).

The kernels train net._w1t (what the scored expansions read) and the module's
own parameters in place, l1.weight as the mirror of _w1t: net(feat),
state_dict() and scored_afterstates(net) agree after every update and no
pack() is needed.

WindowTDLambdaLearner is the windowed form: K plies of
self-play in one launch that writes each ply's record
(narde_value_rollout_records / narde_turn_value_rollout_records), then one
update from the window (narde_value_td_window) with the weights held fixed
over it,
    theta <- theta + alpha sum_e sum_k G_k grad_theta v(s_k),
    G_k = delta_k + gamma lam G_{k+1} (cut where an episode ended, G_K = 0).
It keeps no trace array.  It is truncated TD(lambda), not the online
learner's algorithm: no credit crosses a window's left edge.

ValueFitter is the supervised layer: one update that
regresses given records onto given float targets (narde_value_fit) -- playout
means, lookahead values, anything a caller can compute for a position --,
    theta <- theta + alpha sum_i w_i (target_i - v(s_i)) grad_theta v(s_i).
PlayoutTargetLearner closes the loop with it: a window of self-play, Monte-Carlo
playouts of the window's positions (VecNardeEnv.playout), their means as the
targets (VecNardeEnv.playout_targets), one fit.  LookaheadTargetLearner
 is the same loop with the two-ply values of the window's
positions (VecNardeEnv.lookahead_records) as the targets.

ValueSGD and ValueAdam are optimiser steps on a given
gradient row, on the device.  The three windowed learners and ValueFitter take
optimizer= and grad_hook=: the update then makes the summed gradient
(narde_value_td_window_grad / narde_value_fit_grad; the direction the plain
update moves along, theta += alpha grad), calls grad_hook(grad) -- the place
for an all_reduce over ranks --, and hands it to optimizer.step(grad).  With
neither they run the plain calls as before.
"""
import ctypes

from . import _lib
from .value_net import HIDDEN_ACTS, OUT_ACTS
from .value_play import ValuePlayer


def _need_mlp(name, net):
    """net quacks like a value_net.ValueMLP, or `name`'s TypeError."""
    if not (hasattr(net, "struct") and hasattr(net, "pack")):
        raise TypeError(f"{name} needs a gym_narde.value_net.ValueMLP")


def _check_learner(name, env, net, lam):
    _need_mlp(name, net)
    if not env.autoreset:
        raise ValueError(f"{name} needs an env with autoreset=True")
    if net.l1.weight.device != env.device:
        raise ValueError(f"the net is on {net.l1.weight.device}, the env on {env.device}")
    if not 0.0 <= float(lam) <= 1.0:
        raise ValueError("lam must be in [0, 1]")


def _check_optimizer(name, env, net, alpha, optimizer, grad_hook, alpha_at_step=False):
    """The learners' optimizer= and grad_hook=: an optimiser has the step size
    (alpha must be None with one), is over this net, on this device.
    alpha_at_step: the caller takes alpha with every step, not here."""
    if optimizer is None:
        if grad_hook is not None:
            raise ValueError(f"{name}: grad_hook needs an optimizer (the plain update has no gradient to hand out)")
        if alpha is None and not alpha_at_step:
            raise ValueError(f"{name} needs alpha or an optimizer")
        return
    if not isinstance(optimizer, _ValueOptimizer):
        raise TypeError(f"{name}: optimizer must be a gym_narde.td.ValueSGD or ValueAdam")
    if alpha is not None:
        raise ValueError(f"{name}: alpha and an optimizer are mutually exclusive (the optimizer has the step size); "
                         "pass alpha=None")
    if optimizer.net is not net:
        raise ValueError(f"{name}: the optimizer was made for another net")
    if optimizer.device != env.device:
        raise ValueError(f"the optimizer is on {optimizer.device}, the env on {env.device}")
    if grad_hook is not None and not callable(grad_hook):
        raise TypeError(f"{name}: grad_hook must be callable")


def _train_struct(env, net):
    """The ctypes narde_value_mlp_train over the net's live tensors."""
    return _train_struct_of(env.torch, net)


def _train_struct_of(t, net):
    """_train_struct for a caller without an env (t: the torch module)."""
    net.struct()  # packs _w1t on first use, checks the parameters
    w = net.l1.weight
    if w.dtype != t.float32 or not w.is_contiguous():
        raise ValueError("the learner needs a contiguous float32 l1.weight")
    return _lib.ValueMlpTrain(net._w1t.data_ptr(), net.hidden, net.l1.bias.data_ptr(), net.l2.weight.data_ptr(),
                              net.l2.bias.data_ptr(), net.hidden, HIDDEN_ACTS[net.hidden_act],
                              OUT_ACTS[net.out_act], w.data_ptr(), w.stride(0))


class _ValueOptimizer:
    """What ValueSGD and ValueAdam share: the net's train struct, the gradient
    check, the optional norm clip (narde_value_grad_norm), the stream."""

    def __init__(self, net, max_grad_norm):
        import torch as t

        _need_mlp(type(self).__name__, net)
        if not net.l1.weight.is_cuda:
            raise ValueError(f"{type(self).__name__} needs a net on a GPU device: the steps are device kernels")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError("max_grad_norm must be None or >= 0")
        self.torch, self.net, self.device = t, net, net.l1.weight.device
        self.rows = 200 * net.hidden + 1
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # (norm, clip coefficient) of the last clipped step
        self.norm = None if max_grad_norm is None else t.zeros(2, dtype=t.float32, device=self.device)
        self._mlp = _train_struct_of(t, net)
        self._lib = _lib.load()

    def _s(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _scale(self, grad):
        """Checks grad; with a max_grad_norm the norm launch, and the pointer
        of its coefficient on the device (None: no clip)."""
        t = self.torch
        if (not isinstance(grad, t.Tensor) or grad.dtype != t.float32 or grad.device != self.device
                or not grad.is_contiguous() or tuple(grad.shape) != (self.rows,)):
            raise ValueError(f"grad must be a contiguous ({self.rows},) float32 tensor on {self.device}")
        if self.norm is None:
            return None
        _lib.check(self._lib.narde_value_grad_norm(self.device.index, self.net.hidden, _lib.ptr(grad),
                                                   self.max_grad_norm, _lib.ptr(self.norm), self._s()),
                   "narde_value_grad_norm")
        return ctypes.c_void_p(self.norm.data_ptr() + 4)

    def _load(self, state, names):
        for name in names:
            src, dst = state[name], getattr(self, name)
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"{name}: expected {tuple(dst.shape)} {dst.dtype}, got {tuple(src.shape)} {src.dtype}")
            dst.copy_(src)  # in place: a captured graph keeps its pointers


class ValueSGD(_ValueOptimizer):
    """theta += alpha grad on the device (narde_value_sgd_step): the plain
    updates' own apply, so a learner with ValueSGD(net, alpha) and no clip moves
    the weights to the plain call's bits.  max_grad_norm: clip the row's
    Euclidean norm to it first (torch.nn.utils.clip_grad_norm_'s coefficient).
    step() is stream-ordered and graph-capturable, writes net._w1t and the
    module's parameters alike (no pack()), and makes no synchronise."""

    def __init__(self, net, alpha, max_grad_norm=None):
        super().__init__(net, max_grad_norm)
        if not float(alpha) >= 0.0:
            raise ValueError("alpha must be >= 0")
        self.alpha = float(alpha)
        self.steps = self.torch.zeros((), dtype=self.torch.int64, device=self.device)

    def step(self, grad):
        scale = self._scale(grad)
        _lib.check(self._lib.narde_value_sgd_step(self.device.index, ctypes.byref(self._mlp), _lib.ptr(grad), scale,
                                                  self.alpha, self._s()), "narde_value_sgd_step")
        self.steps += 1

    def state_dict(self):
        return {"steps": self.steps.clone()}

    def load_state_dict(self, state):
        self._load(state, ("steps",))

    def memory_bytes(self):
        """Device memory the optimiser owns."""
        return 8 + (0 if self.norm is None else 8)


class ValueAdam(_ValueOptimizer):
    """torch.optim.AdamW(maximize=True) on the gradient row, on the device
    (narde_value_adam_step); weight_decay = 0 is the papers' Adam.  Owns the
    moments m and s, (200 H + 1,) float32 in the row's layout, and the device
    state -- the step count and the running products beta1^t, beta2^t in
    double --, which a step advances on the device: a captured graph replays
    successive steps.  max_grad_norm: as ValueSGD's.  step() is stream-ordered
    and graph-capturable, writes net._w1t and the module's parameters alike
    (no pack()), and makes no synchronise."""

    def __init__(self, net, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        super().__init__(net, max_grad_norm)
        t = self.torch
        b1, b2 = (float(b) for b in betas)
        if not float(lr) >= 0.0:
            raise ValueError("lr must be >= 0")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("betas must be in [0, 1)")
        if not float(eps) > 0.0:
            raise ValueError("eps must be > 0")
        if not float(weight_decay) >= 0.0:
            raise ValueError("weight_decay must be >= 0")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (b1, b2), float(eps), float(weight_decay)
        self.m = t.zeros(self.rows, dtype=t.float32, device=self.device)
        self.s = t.zeros(self.rows, dtype=t.float32, device=self.device)
        self.state = t.zeros(3, dtype=t.int64, device=self.device)  # narde_adam_state: the count, two doubles

    @property
    def steps(self):
        """The steps taken: a 0-d int64 view of the device state."""
        return self.state[0]

    def beta_pows(self):
        """(beta1^t, beta2^t) as the last step left them: a float64 view."""
        return self.state[1:].view(self.torch.float64)

    def step(self, grad):
        scale = self._scale(grad)
        _lib.check(self._lib.narde_value_adam_step(self.device.index, ctypes.byref(self._mlp), _lib.ptr(grad), scale,
                                                   _lib.ptr(self.m), _lib.ptr(self.s), _lib.ptr(self.state), self.lr,
                                                   self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                                   self._s()), "narde_value_adam_step")

    def state_dict(self):
        return {"m": self.m.clone(), "s": self.s.clone(), "state": self.state.clone()}

    def load_state_dict(self, state):
        self._load(state, ("m", "s", "state"))

    def memory_bytes(self):
        """Device memory the optimiser owns."""
        return 8 * self.rows + 24 + (0 if self.norm is None else 8)


class _SelfPlayWindow:
    """What the three windowed learners share: a window of `plies` plies of
    self-play in one launch, the net on both sides, into buffers with records
    (bufs); the FULL4 launch's scratch (_roll_scratch); the explore pair on
    the device (_eps, _tag: None for greedy play); the count of windows
    played."""

    def _make_window(self, env, net, plies, epsilon, seed):
        t, z = env.torch, dict(device=env.device)
        self.env, self.net, self.plies, self.seed = env, net, int(plies), int(seed)
        self.windows = 0
        self.bufs = env._twin("value_rollout_buffers")(self.plies, records=True)
        self._roll_scratch = env.turn_value_rollout_scratch() if env.full else None
        self._eps = None if epsilon is None else t.tensor(float(epsilon), dtype=t.float32, **z)
        self._tag = None if epsilon is None else t.zeros((), dtype=t.int64, **z)

    def play(self):
        """The window's plies in one launch, the net on both sides; the
        explore tag advances by them.  Returns the launch's buffers."""
        kw = {} if self._roll_scratch is None else dict(scratch=self._roll_scratch)
        self.env._twin("value_rollout")(self.plies, self.net, epsilon=self._eps, tag=self._tag, seed=self.seed,
                                        bufs=self.bufs, **kw)
        if self._tag is not None:
            self._tag += self.plies
        self.windows += 1
        return self.bufs

    def _window_bytes(self):
        own = [x for x in self.bufs.values() if x is not None]
        if self._roll_scratch is not None:
            own.append(self._roll_scratch)
        return sum(x.numel() * x.element_size() for x in own)


class WindowTDLambdaLearner(_SelfPlayWindow):
    """env: a VecNardeEnv (either rule set) with autoreset; net: a ValueMLP on
    its device.  alpha: step size; lam: the return's decay; plies: the
    window K; gamma: the discount; epsilon: the explore probability of the
    play (None: greedy); seed: the explore draws' key.  optimizer: a ValueSGD
    or ValueAdam over the net, alpha then None -- update() makes the window's
    gradient, calls grad_hook(grad) if given (the learner's own (200 H + 1,)
    tensor; edit it in place) and hands it to optimizer.step()."""

    def __init__(self, env, net, alpha, lam, plies, gamma=1.0, epsilon=None, seed=0, optimizer=None, grad_hook=None):
        t = env.torch
        _check_learner("WindowTDLambdaLearner", env, net, lam)
        _check_optimizer("WindowTDLambdaLearner", env, net, alpha, optimizer, grad_hook)
        if int(plies) < 1:
            raise ValueError("plies must be >= 1")
        self._make_window(env, net, plies, epsilon, seed)
        self.alpha = None if alpha is None else float(alpha)
        self.lam, self.gamma = float(lam), float(gamma)
        self.optimizer, self.grad_hook, self.grad = optimizer, grad_hook, None
        z = dict(device=env.device)
        self.delta = t.zeros((self.plies, env.num_envs), dtype=t.float32, **z)
        self.scratch = t.empty(_lib.td_window_scratch_floats(env.num_envs, self.plies, net.hidden), dtype=t.float32, **z)
        self._mlp = _train_struct(env, net)

    def update(self):
        """One weight update from the window play() recorded."""
        if self.optimizer is not None:
            grad = self.gradient()
            if self.grad_hook is not None:
                self.grad_hook(grad)
            self.optimizer.step(grad)
            return
        b = self.bufs
        self.env.handle.call("narde_value_td_window", ctypes.byref(self._mlp), self.plies, _lib.ptr(b["records"]),
                             _lib.ptr(b["reward"]), _lib.ptr(b["terminated"]), _lib.ptr(b["truncated"]), self.alpha,
                             self.lam, self.gamma, _lib.ptr(self.scratch), self.scratch.numel(), _lib.ptr(self.delta),
                             self.env._s())

    def gradient(self):
        """sum_e sum_k G_k grad_theta v(s_k) of the window play() recorded, under
        the weights as they are: (200 H + 1,) float32 in a trace row's layout
        (the learner's own tensor, rewritten by the next call).  Moves no
        weight; delta and values() are the plain update's."""
        b, t = self.bufs, self.env.torch
        if self.grad is None:
            self.grad = t.zeros(200 * self.net.hidden + 1, dtype=t.float32, device=self.env.device)
        self.env.handle.call("narde_value_td_window_grad", ctypes.byref(self._mlp), self.plies, _lib.ptr(b["records"]),
                             _lib.ptr(b["reward"]), _lib.ptr(b["terminated"]), _lib.ptr(b["truncated"]), self.lam,
                             self.gamma, _lib.ptr(self.scratch), self.scratch.numel(), _lib.ptr(self.delta),
                             _lib.ptr(self.grad), self.env._s())
        return self.grad

    def step(self):
        """K plies of self-play and their one update.  Returns (reward,
        terminated, truncated, delta), each [plies][B] (the learner's own
        buffers, rewritten by the next step)."""
        b = self.play()
        self.update()
        return b["reward"], b["terminated"], b["truncated"], self.delta

    def values(self):
        """v (plies + 1, B) of the last update: v(s_k) under the weights it
        found, the last row the envs' records as they stood (a view of the
        scratch)."""
        K, B = self.plies, self.env.num_envs
        return self.scratch[:(K + 1) * B].view(K + 1, B)

    def memory_bytes(self):
        """Device memory the learner owns."""
        own = [self.delta, self.scratch] + ([] if self.grad is None else [self.grad])
        return self._window_bytes() + sum(x.numel() * x.element_size() for x in own)


class ValueFitter:
    """A supervised fit of a ValueMLP on given records and given float
    targets, on the device (narde_value_fit).  env: a VecNardeEnv (its device
    and stream; its positions are not touched); net: a ValueMLP on that
    device; n: the most samples a call takes.  Owns the scratch and the train
    struct; after a step net(feat), state_dict() and scored_afterstates(net)
    agree with no pack(), as with the TD learners.  optimizer: a ValueSGD or
    ValueAdam over the net -- step() then takes no alpha: it makes the
    gradient, calls grad_hook(grad) if given and hands it to optimizer.step()."""

    def __init__(self, env, net, n, optimizer=None, grad_hook=None):
        t = env.torch
        _need_mlp("ValueFitter", net)
        if net.l1.weight.device != env.device:
            raise ValueError(f"the net is on {net.l1.weight.device}, the env on {env.device}")
        if int(n) < 1:
            raise ValueError("n must be >= 1")
        _check_optimizer("ValueFitter", env, net, None, optimizer, grad_hook, alpha_at_step=True)
        self.env, self.net, self.n = env, net, int(n)
        self.optimizer, self.grad_hook, self.grad = optimizer, grad_hook, None
        z = dict(device=env.device)
        self.scratch = t.empty(_lib.value_fit_scratch_floats(self.n, net.hidden), dtype=t.float32, **z)
        self.v = t.zeros(self.n, dtype=t.float32, **z)
        self.loss = t.zeros(2, dtype=t.float64, **z)
        self._m = 0
        self._mlp = _train_struct(env, net)

    def step(self, records, target, weight=None, *, alpha=None):
        """theta += alpha sum_i w_i (target_i - v(s_i)) grad v(s_i): a sum, not
        a mean (divide alpha by the weights' sum for that).  records (m, 8)
        int32 (state_records(), a records rollout's, recorded rows'), m <= n;
        target (m,) float32 white's values to regress to; weight (m,) float32
        or None (all 1) -- where it is 0 the target is never read.  Returns
        the device tensor loss (2,) float64 = (sum w e^2, sum w) under the
        weights the call found (the fitter's own, rewritten by the next call).
        No synchronise.  A fitter with an optimizer takes no alpha: the sum
        goes through grad_hook to optimizer.step()."""
        if self.optimizer is None:
            if alpha is None:
                raise TypeError("ValueFitter.step() needs alpha= (the fitter has no optimizer)")
            return self._call(records, target, weight, float(alpha), False)
        if alpha is not None:
            raise ValueError("ValueFitter.step(): alpha and an optimizer are mutually exclusive (the optimizer has the "
                             "step size)")
        grad = self.gradient(records, target, weight)
        if self.grad_hook is not None:
            self.grad_hook(grad)
        self.optimizer.step(grad)
        return self.loss

    def gradient(self, records, target, weight=None):
        """sum_i w_i (target_i - v(s_i)) grad v(s_i) under the weights as they
        are: (200 H + 1,) float32 in a trace row's layout (the fitter's own
        tensor, rewritten by the next call).  Moves no weight; loss and
        values() are step()'s."""
        t = self.env.torch
        if self.grad is None:
            self.grad = t.zeros(200 * self.net.hidden + 1, dtype=t.float32, device=self.env.device)
        self._call(records, target, weight, 0.0, True)
        return self.grad

    def _call(self, records, target, weight, alpha, to_grad):
        t, env = self.env.torch, self.env
        if (not isinstance(records, t.Tensor) or records.dtype != t.int32 or records.device != env.device
                or not records.is_contiguous() or records.dim() != 2 or records.shape[1] != 8):
            raise ValueError("records must be a contiguous (m, 8) int32 device tensor")
        m = int(records.shape[0])
        if not 1 <= m <= self.n:
            raise ValueError(f"{m} samples: the fitter was made for 1 .. {self.n}")
        target = env._dev(target, t.float32, (m,))
        weight = None if weight is None else env._dev(weight, t.float32, (m,))
        if to_grad:
            _lib.check(env.handle.lib.narde_value_fit_grad(env.device.index, ctypes.byref(self._mlp), m,
                                                           _lib.ptr(records), _lib.ptr(target), _lib.ptr(weight),
                                                           _lib.ptr(self.scratch), self.scratch.numel(),
                                                           _lib.ptr(self.v), _lib.ptr(self.loss), _lib.ptr(self.grad),
                                                           env._s()), "narde_value_fit_grad")
        else:
            _lib.check(env.handle.lib.narde_value_fit(env.device.index, ctypes.byref(self._mlp), m, _lib.ptr(records),
                                                      _lib.ptr(target), _lib.ptr(weight), float(alpha),
                                                      _lib.ptr(self.scratch), self.scratch.numel(), _lib.ptr(self.v),
                                                      _lib.ptr(self.loss), env._s()), "narde_value_fit")
        self._m, self._keep = m, (records, target, weight)
        return self.loss

    def evaluate(self, records, target, weight=None):
        """The plain call with alpha = 0: the loss and values(), no weight bit
        moved (with or without an optimizer)."""
        return self._call(records, target, weight, 0.0, False)

    def values(self):
        """v (m,) of the last call: v(s_i) under the weights it found."""
        return self.v[:self._m]

    def memory_bytes(self):
        """Device memory the fitter owns."""
        own = [self.scratch, self.v, self.loss] + ([] if self.grad is None else [self.grad])
        return sum(x.numel() * x.element_size() for x in own)


class PlayoutTargetLearner(_SelfPlayWindow):
    """Self-play, playouts of its positions, a fit onto their means (DESIGN.md
    section 24).  env: a VecNardeEnv (either rule set) with autoreset; net: a
    ValueMLP on its device.  Every step: play() -- `plies` plies of
    value-greedy self-play in one launch that records each ply's position;
    targets() -- the positions of plies k % every == 0, N = ceil(plies / every)
    * B roots, each played out `trials` times to the end (max_plies plies at
    most) under playout_net on both colours (None: the net itself), the roots'
    mean outcomes the targets; update() -- one narde_value_fit of those roots
    at step size alpha (a sum over the roots).  Without leaf a root none of
    whose trials finished gets weight 0.  With leaf=True an unfinished trial
    counts at the net's value of the position it stopped at: with a small
    max_plies that is an n-step truncated-rollout target, a bootstrap max_plies
    plies deep instead of a Monte-Carlo return.  epsilon: the explore
    probability of the self-play (None: greedy); common_dice: playout()'s.
    The playouts' seed is seed + the count of windows played: the same
    arguments and the same number of steps give the same weight bits.
    optimizer, grad_hook: ValueFitter's (alpha then None)."""

    def __init__(self, env, net, alpha, plies, trials, every=1, max_plies=400, leaf=False, playout_net=None,
                 epsilon=None, common_dice=False, seed=0, optimizer=None, grad_hook=None):
        t = env.torch
        _check_learner("PlayoutTargetLearner", env, net, 0.0)
        _check_optimizer("PlayoutTargetLearner", env, net, alpha, optimizer, grad_hook)
        if int(plies) < 1 or int(trials) < 1 or int(every) < 1 or int(max_plies) < 1:
            raise ValueError("plies, trials, every and max_plies must be >= 1")
        self._make_window(env, net, plies, epsilon, seed)
        self.trials, self.every, self.max_plies, self.leaf = int(trials), int(every), int(max_plies), bool(leaf)
        self.playout_net = net if playout_net is None else playout_net
        self.alpha = None if alpha is None else float(alpha)
        self.common_dice = bool(common_dice)
        z = dict(device=env.device)
        B, M = env.num_envs, -(-self.plies // self.every)
        N = M * B
        self.roots = t.zeros((N, 8), dtype=t.int32, **z)
        self.result = None  # the playouts' PlayoutResult, made by the first targets()
        self.target = t.zeros(N, dtype=t.float32, **z)
        self.weight = t.zeros(N, dtype=t.float32, **z)
        self.fitter = ValueFitter(env, net, N, optimizer=optimizer, grad_hook=grad_hook)

    def targets(self):
        """Playouts of the window's positions and their targets.  Returns
        (target, weight), each (N,), root j * B + e = env e before ply j *
        every (the learner's own buffers)."""
        env, B = self.env, self.env.num_envs
        self.roots.view(-1, B, 8).copy_(self.bufs["records"][::self.every])
        self.result = env.playout(self.roots, self.trials, self.playout_net, max_plies=self.max_plies,
                                  seed=self.seed + self.windows, common_dice=self.common_dice, leaf=self.leaf,
                                  out=self.result)
        return env.playout_targets(self.result, roots=self.roots, leaf=self.leaf, out=(self.target, self.weight))

    def update(self):
        """One fit of the roots onto targets()' numbers.  Returns the loss
        (2,) float64 = (sum w e^2, sum w) under the weights it found."""
        return self.fitter.step(self.roots, self.target, self.weight, alpha=self.alpha)

    def step(self):
        """play(), targets(), update().  Returns (loss, target, weight)."""
        self.play()
        self.targets()
        return self.update(), self.target, self.weight

    def values(self):
        """v (N,) of the last update, under the weights it found."""
        return self.fitter.values()

    def memory_bytes(self):
        """Device memory the learner owns."""
        own = [self.roots, self.target, self.weight]
        if self.result is not None:
            own += [x for x in (self.result.sums, self.result.outcome, self.result.length, self.result.leaf)
                    if x is not None]
        return self._window_bytes() + sum(x.numel() * x.element_size() for x in own) + self.fitter.memory_bytes()


class LookaheadTargetLearner(_SelfPlayWindow):
    """Self-play and a fit onto the two-ply values of its positions (DESIGN.md
    section 25): PlayoutTargetLearner with VecNardeEnv.lookahead_records() in
    place of the playouts.  env: a VecNardeEnv (either rule set) with
    autoreset; net: a ValueMLP on its device.  Every step: play() -- `plies`
    plies of value-greedy self-play in one launch that records each ply's
    position; targets() -- the positions of plies k % every == 0, N =
    ceil(plies / every) * B roots, each root's target its two-ply value under
    the net (the expectation, over its mover's rolls, of the mover's best
    afterstate), its weight 1 -- 0 where that value is NaN (a finished
    position); update() -- one narde_value_fit of those roots at step size
    alpha (a sum over the roots).  epsilon: the explore probability of the
    self-play (None: greedy).  Nothing is drawn besides the self-play: the same
    arguments and the same number of steps give the same weight bits.
    optimizer, grad_hook: ValueFitter's (alpha then None)."""

    def __init__(self, env, net, alpha, plies, every=1, epsilon=None, seed=0, optimizer=None, grad_hook=None):
        t = env.torch
        _check_learner("LookaheadTargetLearner", env, net, 0.0)
        _check_optimizer("LookaheadTargetLearner", env, net, alpha, optimizer, grad_hook)
        if int(plies) < 1 or int(every) < 1:
            raise ValueError("plies and every must be >= 1")
        self._make_window(env, net, plies, epsilon, seed)
        self.every, self.alpha = int(every), None if alpha is None else float(alpha)
        z = dict(device=env.device)
        B, M = env.num_envs, -(-self.plies // self.every)
        N = M * B
        self.roots = t.zeros((N, 8), dtype=t.int32, **z)
        self.target = t.zeros(N, dtype=t.float32, **z)
        self.weight = t.zeros(N, dtype=t.float32, **z)
        self.fitter = ValueFitter(env, net, N, optimizer=optimizer, grad_hook=grad_hook)

    def targets(self):
        """The two-ply values of the window's positions.  Returns (target,
        weight), each (N,), root j * B + e = env e before ply j * every (the
        learner's own buffers); target NaN, weight 0, for a finished root."""
        env, B, t = self.env, self.env.num_envs, self.env.torch
        self.roots.view(-1, B, 8).copy_(self.bufs["records"][::self.every])
        env.lookahead_records(self.roots, self.net, out=self.target)
        self.weight.copy_(~t.isnan(self.target))
        return self.target, self.weight

    def update(self):
        """One fit of the roots onto targets()' numbers.  Returns the loss
        (2,) float64 = (sum w e^2, sum w) under the weights it found."""
        return self.fitter.step(self.roots, self.target, self.weight, alpha=self.alpha)

    def step(self):
        """play(), targets(), update().  Returns (loss, target, weight)."""
        self.play()
        self.targets()
        return self.update(), self.target, self.weight

    def values(self):
        """v (N,) of the last update, under the weights it found."""
        return self.fitter.values()

    def memory_bytes(self):
        """Device memory the learner owns (the env keeps lookahead_records()'
        scratch of a rules="full4" env)."""
        own = [self.roots, self.target, self.weight]
        return self._window_bytes() + sum(x.numel() * x.element_size() for x in own) + self.fitter.memory_bytes()


class TDLambdaLearner:
    """env: a VecNardeEnv (either rule set) with autoreset; net: a ValueMLP on
    its device.  alpha: step size; lam: the trace decay; gamma: the discount;
    epsilon: the explore probability of the play (None: greedy); cap: the
    rows a ply's expansion holds (ValuePlayer's: with it a step makes no
    synchronise)."""

    def __init__(self, env, net, alpha, lam, gamma=1.0, epsilon=None, seed=0, cap=None):
        t = env.torch
        _need_mlp("TDLambdaLearner", net)
        if not env.autoreset:
            raise ValueError("TDLambdaLearner needs an env with autoreset=True")
        if net.l1.weight.device != env.device:
            raise ValueError(f"the net is on {net.l1.weight.device}, the env on {env.device}")
        if not 0.0 <= float(lam) <= 1.0:
            raise ValueError("lam must be in [0, 1]")
        self.env, self.net = env, net
        self.alpha, self.lam, self.gamma, self.seed = float(alpha), float(lam), float(gamma), int(seed)
        B, H = env.num_envs, net.hidden
        self.row_floats = 200 * H + 1
        self.ld_trace = (self.row_floats + 3) // 4 * 4
        need = B * self.ld_trace * 4
        free = t.cuda.mem_get_info(env.device)[0]
        if need > free:
            raise ValueError(f"{B} envs x {self.ld_trace} trace floats = {need / 1e6:.0f} MB exceed the device's free "
                             f"memory ({free / 1e6:.0f} MB): use fewer envs or a smaller hidden layer")
        z = dict(device=env.device)
        self.trace = t.zeros((B, self.ld_trace), dtype=t.float32, **z)
        self.v = t.zeros(B, dtype=t.float32, **z)
        self.black = t.zeros(B, dtype=t.uint8, **z)
        self.delta = t.zeros(B, dtype=t.float32, **z)
        self.scratch = t.empty(_lib.td_scratch_floats(B, H), dtype=t.float32, **z)
        self.player = ValuePlayer(env, net, perspective="white", fused=True, cap=cap)
        self._eps = None if epsilon is None else t.tensor(float(epsilon), dtype=t.float32, **z)
        self._tag = None if epsilon is None else t.zeros((), dtype=t.int64, **z)
        self._mlp = self.struct()

    def struct(self):
        """The ctypes narde_value_mlp_train over the net's live tensors."""
        return _train_struct(self.env, self.net)

    def trace_pass(self, decay=None):
        """v, black and the traces from the envs' records as they stand."""
        decay = self.gamma * self.lam if decay is None else float(decay)
        self.env.handle.call("narde_value_td_trace", ctypes.byref(self._mlp), decay, _lib.ptr(self.trace),
                             self.ld_trace, _lib.ptr(self.v), _lib.ptr(self.black), self.env._s())

    def apply_pass(self, reward, terminated, truncated):
        """The update after the step (its reward, terminated, truncated)."""
        self.env.handle.call("narde_value_td_apply", ctypes.byref(self._mlp), _lib.ptr(self.trace), self.ld_trace,
                             _lib.ptr(self.v), _lib.ptr(self.black), _lib.ptr(reward), _lib.ptr(terminated),
                             _lib.ptr(truncated), self.alpha, self.gamma, 1, _lib.ptr(self.scratch),
                             self.scratch.numel(), _lib.ptr(self.delta), self.env._s())

    def step(self):
        """One ply of self-play and its update.  Returns ValuePlayer.step's
        tuple plus delta (B,) float32, the ply's TD errors."""
        self.trace_pass()
        if self._eps is None:
            out = self.player.step()
        else:
            out = self.player.step(epsilon=self._eps, tag=self._tag, seed=self.seed)
            self._tag += 1
        self.apply_pass(out[1], out[2], out[3])
        return out + (self.delta,)

    def traces(self):
        """The traces shaped like the module's parameters with a leading B
        (views of the learner's buffer)."""
        B, H = self.env.num_envs, self.net.hidden
        tr = self.trace
        return {"l1.weight": tr[:, :198 * H].reshape(B, 198, H).transpose(1, 2),
                "l1.bias": tr[:, 198 * H:199 * H],
                "l2.weight": tr[:, 199 * H:200 * H].reshape(B, 1, H),
                "l2.bias": tr[:, 200 * H:200 * H + 1]}

    def memory_bytes(self):
        """Device memory the learner owns."""
        return sum(x.numel() * x.element_size() for x in (self.trace, self.v, self.black, self.delta, self.scratch))
