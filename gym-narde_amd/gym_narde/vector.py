"""VecNardeEnv -- B Narde envs stepped in lockstep on one GPU.

This is the batched hot path the scalar NardeEnv (narde_env.py:27-103 of the
reference) is replaced by: state stays resident in HBM (32 B/env), every call
is one stream-ordered kernel launch on the caller's current torch stream, and
outputs land in preallocated device tensors (valid until the next call of the
same kind -- clone them to keep them).

Dice of ply t for global env e are Philox4x32-10({t, e, 0, 0}, seed), so
`dice()` / `legal_moves()` / `legal_mask()` describe exactly the roll the next
`step()` will use (the reference's callers peek/roll their own dice instead,
train_deepq_pytorch.py:866).  Actions are the reference's codes
(from*24 + to, (from<=5, to==0) = bear-off).

rules="ref2" (default) is the reference's NardeEnv.step: at most two checker
moves per step, quirks included.  rules="full4" is the build's whole-turn
mode (include/narde.h): four sub-moves on doubles, max
dice used, the higher die when only one can be used.  Its actions are plays,
(B,4,2) int8 (from, die) sub-moves; info["legal"] is the first sub-move's
set with the max dice usable in bits 56-58, info["played"] the sub-moves
played (bytes 2k/2k+1 = from/die, 0xFF unused).
"""
import collections
import ctypes
import os
import weakref

import numpy as np

from . import _lib

DICE_MODES = {"all36": _lib.DICE_ALL36, "nodoubles": _lib.DICE_NODOUBLES}
RULES = ("ref2", "full4")


def decode_compact(compact):
    """Compact legal set(s) (u64, see include/narde.h) -> list(s) of (from, to)
    with to == 'off' for bear-off, in the reference's list order."""
    arr = np.atleast_1d(np.asarray(compact, dtype=np.uint64))
    out = []
    for c in arr.tolist():
        lh, ll = c & 0xFFFFFF, (c >> 24) & 0xFFFFFF
        dh, dl = (c >> 48) & 0xF, (c >> 52) & 0xF
        moves = []
        for L, d in ((lh, dh), (ll, dl)):
            if d == 0:
                continue
            for p in range(24):
                if (L >> p) & 1:
                    moves.append((p, "off" if p - d < 0 else p - d))
        out.append(moves)
    return out if np.ndim(compact) else out[0]


def decode_full_legal(word):
    """FULL4 legal word (u64) -> (max_dice, [(from, die), ...]) in list
    order (higher die first, ascending source)."""
    c = int(np.uint64(word))
    ch, cl = c & 0xFFFFFF, (c >> 24) & 0xFFFFFF
    dh, dl, m = (c >> 48) & 0xF, (c >> 52) & 0xF, (c >> 56) & 0x7
    opts = [(p, dh) for p in range(24) if (ch >> p) & 1]
    if dl != dh:
        opts += [(p, dl) for p in range(24) if (cl >> p) & 1]
    return m, opts


def decode_played(word):
    """FULL4 played word (u64) -> [(from, die), ...] sub-moves in order."""
    c = int(np.uint64(word))
    out = []
    for k in range(4):
        f, d = (c >> (16 * k)) & 0xFF, (c >> (16 * k + 8)) & 0xFF
        if f == 0xFF:
            break
        out.append((f, d))
    return out


PLAY_KINDS = {"act": 0, "step": 1}


def decode_play_set(legal, words, kind="act"):
    """One env's play set (VecNardeEnv.play_set: its compact list #1 and
    its (2, 24) entry words) in the reference's terms.
    kind "act": DQNAgent.act's valid_move_combinations
    (train_deepq_pytorch.py:430-507) -- a list of (move1_code, move2_code)
    in act()'s order, duplicates included ('off' coded as to = 0, no second
    move as 0).  kind "step": the set of plays NardeEnv.step carries out
    (narde_env.py:45-93) as move tuples ((m1, m2), or (m1,) alone), as
    Narde.get_valid_plays returns them."""
    c = int(np.uint64(np.int64(legal)))
    w = np.asarray(words).astype(np.int64).reshape(2, 24)
    masks = (c & 0xFFFFFF, (c >> 24) & 0xFFFFFF)
    dies = ((c >> 48) & 0xF, (c >> 52) & 0xF)
    entries = [(k, p, dies[k]) for k in range(2) if dies[k] for p in range(24) if (masks[k] >> p) & 1]
    out = [] if kind == "act" else set()
    for k, p, d in entries:
        wd = int(w[k, p])
        m2, rem = wd & 0xFFFFFF, (wd >> 24) & 7
        seconds = [(q, "off" if q < rem else q - rem) for q in range(24) if (m2 >> q) & 1]
        m1 = (p, "off" if p < d else p - d)
        if kind == "act":
            c1 = p * 24 + (0 if m1[1] == "off" else m1[1])
            if not seconds:
                out.append((c1, 0))
            for q, t in seconds:
                out.append((c1, q * 24 + (0 if t == "off" else t)))
        elif len(entries) == 1 or not seconds:
            out.add((m1,))
        else:
            out.update((m1, m2_) for m2_ in seconds)
    return out


PERSPECTIVES = {"mover": 0, "white": 1}

# VecNardeEnv.afterstates' result: CSR rows (env e's rows are offsets[e] ..
# offsets[e + 1] - 1); cap = the rows the arrays hold -- offsets[B] > cap
# means the call overflowed and the rows from cap on were not written
Afterstates = collections.namedtuple("Afterstates", "offsets row_env codes feat obs reward cap")
# VecNardeEnv.turn_afterstates' result (rules="full4"): the same CSR rows with
# play (R,4,2) int8 (from, die) in place of the action codes
TurnAfterstates = collections.namedtuple("TurnAfterstates", "offsets row_env play feat obs reward cap")
# a rule set as the Python surface sees it (an env's is self._kind): the result
# tuple; the action column (field, trailing shape, torch dtype) and the picks'
# fill for no row; the C entry point of every call that has a REF2 / FULL4 twin
# (expand + "_scored" / "_lookahead" / "_records" are its other forms); whether
# the twins of the rollouts, playouts and records lookahead take a scratch (the
# FULL4 ones do); the lookahead's scratch size;
# the value rollouts' [plies][B] buffers (name, trailing shape, torch dtype);
# the public methods that are a REF2 method's twin, by that method's name
# (VecNardeEnv._twin(), for callers that serve both rule sets)
_RowKind = collections.namedtuple(
    "_RowKind", "tuple field shape dtype no_row expand pick playout_pick slot_pick records_lookahead value_rollout "
                "league playout step selfplay rollout turn_scratch look_scratch bufs twins")
_TWINS = ("afterstates", "scored_afterstates", "lookahead_afterstates", "recorded_afterstates", "pick_afterstate",
          "value_rollout", "value_rollout_buffers", "value_rollout_league")
_RECORDS_BUF = ("records", (8,), "int32")


_REF2_ROWS = _RowKind(
    tuple=Afterstates, field="codes", shape=(2,), dtype="int16", no_row=0,
    expand="narde_afterstates", pick="narde_afterstate_pick", playout_pick="narde_playout_pick",
    slot_pick="narde_slot_pick", records_lookahead="narde_records_lookahead",
    value_rollout="narde_value_rollout_records", league="narde_value_rollout_league", playout="narde_value_playout",
    step="narde_step", selfplay="narde_selfplay", rollout="narde_rollout",
    turn_scratch=False, look_scratch=_lib.lookahead_scratch_bytes,
    bufs=(("dice", (2,), "uint8"), ("actions", (2,), "int16"), ("value", (), "float32"), ("reward", (), "int32"),
          ("terminated", (), "uint8"), ("truncated", (), "uint8")),
    twins=dict(zip(_TWINS, _TWINS)))
_FULL4_ROWS = _RowKind(
    tuple=TurnAfterstates, field="play", shape=(4, 2), dtype="int8", no_row=-1,
    expand="narde_turn_afterstates", pick="narde_turn_pick", playout_pick="narde_turn_playout_pick",
    slot_pick="narde_turn_slot_pick", records_lookahead="narde_turn_records_lookahead",
    value_rollout="narde_turn_value_rollout_records", league="narde_turn_value_rollout_league",
    playout="narde_turn_value_playout", step="narde_step_full", selfplay="narde_selfplay_full",
    rollout="narde_rollout_full",
    turn_scratch=True, look_scratch=_lib.turn_lookahead_scratch_bytes,
    bufs=(("dice", (2,), "uint8"), ("play", (4, 2), "int8"), ("value", (), "float32"), ("reward", (), "int32"),
          ("terminated", (), "uint8"), ("truncated", (), "uint8")),
    twins=dict(zip(_TWINS, ("turn_afterstates", "scored_turn_afterstates", "lookahead_turn_afterstates",
                            "recorded_turn_afterstates", "pick_turn", "turn_value_rollout",
                            "turn_value_rollout_buffers", "turn_value_rollout_league"))))


_SAME = object()  # value_rollout(): "net_black is net_white"


class PlayoutResult:
    """VecNardeEnv.playout()'s result for N roots of `trials` trials each:
    sums (N, 4) int32 -- its columns finished (trials that reached the end),
    points (the sum of white's outcomes, each +-1 or +-2), squares (the sum of
    their squares) and plies (played by all trials) --, and the optional
    per-trial outcome (N, trials) int8, length (N, trials) int32 and leaf
    (N, trials) float32 (white's value where a trial stopped unfinished, NaN
    where it finished).  Device tensors; reading them synchronises."""

    def __init__(self, sums, trials, outcome=None, length=None, leaf=None):
        self.sums, self.trials = sums, int(trials)
        self.outcome, self.length, self.leaf = outcome, length, leaf

    finished = property(lambda self: self.sums[:, 0])
    points = property(lambda self: self.sums[:, 1])
    squares = property(lambda self: self.sums[:, 2])
    plies = property(lambda self: self.sums[:, 3])

    def mean(self, truncated=False):
        """White's mean outcome per root, float64: over the finished trials
        (NaN where none finished), or with truncated=True over all trials, an
        unfinished one counted at its leaf value: (points +
        nansum(leaf)) / trials, summed in index order."""
        import torch

        pts = self.points.double()
        if not truncated:
            return pts / self.finished.double()
        if self.leaf is None:
            raise ValueError("mean(truncated=True) needs playout(leaf=True)")
        return (pts + torch.nansum(self.leaf.cpu().double(), dim=1).to(pts.device)) / self.trials

    def stderr(self):
        """The standard error of mean() over the finished trials, float64
        (NaN with fewer than two)."""
        f, pts, sq = self.finished.double(), self.points.double(), self.squares.double()
        var = (sq - pts * pts / f) / (f - 1.0)
        return (var.clamp(min=0.0) / f).sqrt().masked_fill(f < 2.0, float("nan"))


class VecNardeEnv:
    def __init__(self, num_envs, device=None, seed=0, env_id_offset=0, dice_mode="all36",
                 max_episode_steps=1000, autoreset=True, rules="ref2"):
        import torch

        if rules not in RULES:
            raise ValueError(f"rules must be one of {RULES}")
        self.rules = rules
        self.full = rules == "full4"

        self.torch = torch
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise ValueError("VecNardeEnv runs on a GPU device only")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.num_envs = int(num_envs)
        self.autoreset = bool(autoreset)
        self.handle = _lib.Handle(dev.index, num_envs, env_id_offset, seed, DICE_MODES[dice_mode],
                                  max_episode_steps)
        B = self.num_envs
        z = dict(device=dev)
        self.obs = torch.zeros((B, 24), dtype=torch.int32, **z)
        self.reward = torch.zeros(B, dtype=torch.int32, **z)
        self.terminated = torch.zeros(B, dtype=torch.uint8, **z)
        self.truncated = torch.zeros(B, dtype=torch.uint8, **z)
        self.legal = torch.zeros(B, dtype=torch.int64, **z)
        self.actions_used = torch.zeros((B, 2), dtype=torch.int16, **z)
        self.played = torch.zeros(B, dtype=torch.int64, **z)
        self._look_scratch = None  # the lookahead calls' row records, made on the first call
        self._bind()

    # ------------------------------------------------------------ plumbing
    def _bind(self):
        """What __init__ resolves once from the rule set, the handle and the
        step buffers: the rule set's descriptor, and the per-call plumbing of
        step() -- the bound entry point and the output buffers' pointers (they
        never move).  (A method of its own so that a host-only test double,
        which cannot run __init__, resolves them the same way.)"""
        self._kind = k = _FULL4_ROWS if self.full else _REF2_ROWS
        # the value rollouts' buffers as the launches check them: (name, torch dtype, shape behind plies, dtype's name)
        self._buf_specs = tuple((name, getattr(self.torch, dt), (self.num_envs,) + shape, dt)
                                for name, shape, dt in k.bufs + (_RECORDS_BUF,))
        self._step_fn = getattr(self.handle.lib, self._kind.step)
        self._step_out = tuple(_lib.ptr(t) for t in (self.obs, self.reward, self.terminated, self.truncated, self.legal,
                                                     self.played if self.full else self.actions_used))

    def _s(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype, shape):
        if (isinstance(x, self.torch.Tensor) and x.dtype == dtype and x.device == self.device
                and x.is_contiguous() and tuple(x.shape) == tuple(shape)):
            return x  # already a device tensor of the right layout
        t = self.torch.as_tensor(x, device=self.device).to(dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _twin(self, name):
        """The env's method for its rule set that is the REF2 method `name`
        or its FULL4 twin (for td.py and value_play.py, which serve both)."""
        return getattr(self, self._kind.twins[name])

    @property
    def ply(self):
        return self.handle.ply

    @ply.setter
    def ply(self, t):
        self.handle.ply = t

    # ------------------------------------------------------------ API
    def reset(self, mask=None, opening=None):
        """NardeEnv.reset (narde_env.py:105-120) for all (or the masked) envs;
        returns obs (B,24) int32.  opening: (B,K,2) uint8 opening draws
        (white roll, black roll) per env in the reference's draw order -- the
        first pair of different dice decides who moves first, pairs with a
        die outside 1..6 are padding -- or None for the device draw (also
        for an env whose row has no deciding pair)."""
        B = self.num_envs
        m = None if mask is None else self._dev(mask, self.torch.uint8, (B,))
        o, pairs = None, 0
        if opening is not None:
            o = self.torch.as_tensor(opening, device=self.device).to(self.torch.uint8).contiguous()
            if o.dim() == 2:
                o = o.reshape(B, 1, 2)
            if o.dim() != 3 or o.shape[0] != B or o.shape[2] != 2 or o.shape[1] < 1:
                raise ValueError(f"opening must be (B, K, 2) with B = {B}, got {tuple(o.shape)}")
            pairs = int(o.shape[1])
        self.handle.call("narde_reset", _lib.ptr(m), _lib.ptr(o), pairs, self._s())
        self._keep = (m, o)  # inputs alive until the kernel has read them
        return self.observe()

    def observe(self):
        self.handle.call("narde_observe", _lib.ptr(self.obs), None, self._s())
        return self.obs

    def tesauro198(self, out=None):
        """README.md:42-102 198-float observation, (B,198) float32."""
        if out is None:
            out = self.torch.empty((self.num_envs, 198), dtype=self.torch.float32, device=self.device)
        self.handle.call("narde_observe", None, _lib.ptr(out), self._s())
        return out

    def observe_host(self, kind="int24", out=None):
        """Observations for CPU-side agents:
        the observe kernel writes the device buffer and a non-blocking copy
        lands it in PINNED host memory on the same stream.  Returns (host
        tensor, event); read the host tensor after event.synchronize().
        kind: "int24" (the reference's int32[24] obs) or "tesauro198"."""
        t = self.torch
        if kind == "int24":
            dev, shape, dt = self.observe(), (self.num_envs, 24), t.int32
        elif kind == "tesauro198":
            dev, shape, dt = self.tesauro198(), (self.num_envs, 198), t.float32
        else:
            raise ValueError("kind must be 'int24' or 'tesauro198'")
        if out is None:
            out = t.empty(shape, dtype=dt, pin_memory=True)
        elif tuple(out.shape) != shape or out.dtype != dt or not out.is_pinned():
            raise ValueError(f"out must be a pinned {dt} tensor of shape {shape}")
        out.copy_(dev, non_blocking=True)
        ev = t.cuda.Event()
        ev.record(t.cuda.current_stream(self.device))
        self._keep_host = dev  # the source stays alive until the copy is done
        return out, ev

    def dice(self):
        """Dice of the next device-RNG step, (B,2) uint8 in roll order."""
        d = self.torch.empty((self.num_envs, 2), dtype=self.torch.uint8, device=self.device)
        self.handle.call("narde_peek_dice", _lib.ptr(d), self._s())
        return d

    def legal_moves(self, dice=None, expanded=True):
        """Narde.get_valid_moves per env.  dice: (B,k) k<=4 (0 = unused) or None
        for the next step's dice.  Returns (count (B,) int16, moves (B,64,2)
        int8 or None, compact (B,) int64 or None)."""
        B = self.num_envs
        d4 = None
        if dice is not None:
            d = self.torch.as_tensor(dice, device=self.device).to(self.torch.uint8)
            d4 = self.torch.zeros((B, 4), dtype=self.torch.uint8, device=self.device)
            d4[:, : d.shape[1]] = d
        count = self.torch.empty(B, dtype=self.torch.int16, device=self.device)
        moves = (self.torch.empty((B, _lib.MAX_MOVES, 2), dtype=self.torch.int8, device=self.device)
                 if expanded else None)
        # compact form is only defined for <= 2 dice (the kernel writes 0 otherwise)
        compact = self.torch.empty(B, dtype=self.torch.int64, device=self.device)
        self.handle.call("narde_legal_moves", _lib.ptr(d4), _lib.ptr(count), _lib.ptr(moves),
                         _lib.ptr(compact), self._s())
        return count, moves, compact

    def legal_mask(self, out=None):
        """(B,9) int64 = 576-bit mask of move1 codes the next step accepts."""
        if out is None:
            out = self.torch.empty((self.num_envs, 9), dtype=self.torch.int64, device=self.device)
        self.handle.call("narde_legal_mask576", _lib.ptr(out), self._s())
        return out

    def legal_mask_move2(self, move1, dice=None, out=None):
        """(B,9) int64 = 576-bit mask of move2 codes step() accepts after the
        move1 codes (B,), for dice (B,2) or the next step's device dice (all
        zero where move1 would not be played)."""
        B = self.num_envs
        m1 = self._dev(move1, self.torch.int16, (B,))
        d = None if dice is None else self._dev(dice, self.torch.uint8, (B, 2))
        if out is None:
            out = self.torch.empty((B, 9), dtype=self.torch.int64, device=self.device)
        self.handle.call("narde_legal_mask576_move2", _lib.ptr(m1), _lib.ptr(d), _lib.ptr(out),
                         self._s())
        self._keep = (m1, d)
        return out

    def play_set(self, dice=None, kind="act"):
        """The plays of each env's two-dice roll (narde_play_set; the
        README's get_valid_actions, README.md:156-165) for dice (B,2) in roll
        order or the next step's device dice.  Returns (legal (B,) int64
        compact list #1, words (B,2,24) int32 -- per list-#1 entry its
        second-move sources | rem << 24 | 1 << 27, count (B,) int32 plays).
        kind "act": DQNAgent.act's combinations, second moves on the
        PRE-move board (train_deepq_pytorch.py:430-507); "step": the plays
        NardeEnv.step carries out, second moves on the POST-move board
        (narde_env.py:45-93).  decode_play_set() turns one env's row into
        the reference's list / set."""
        if kind not in PLAY_KINDS:
            raise ValueError(f"kind must be one of {tuple(PLAY_KINDS)}")
        B, t = self.num_envs, self.torch
        d = None if dice is None else self._dev(dice, t.uint8, (B, 2))
        legal = t.empty(B, dtype=t.int64, device=self.device)
        words = t.empty((B, 2, 24), dtype=t.int32, device=self.device)
        count = t.empty(B, dtype=t.int32, device=self.device)
        self.handle.call("narde_play_set", _lib.ptr(d), PLAY_KINDS[kind], _lib.ptr(legal), _lib.ptr(words),
                         _lib.ptr(count), self._s())
        self._keep = (d,)
        return legal, words, count

    def act_masks(self, move1=None, dice=None, out=None):
        """DQNAgent.act's greedy candidate sets (narde_act_masks) as (B,9)
        int64 576-bit masks: move1 None -- the move-1 codes of list #1
        (valid_first_moves' keys); move1 (B,) int64 (any positive stride)
        -- the move-2 codes act() offers after it (the pre-move second list
        of the last list-#1 entry with that code; code 0 alone if empty)."""
        B, t = self.num_envs, self.torch
        d = None if dice is None else self._dev(dice, t.uint8, (B, 2))
        if move1 is not None and (move1.dtype != t.int64 or move1.dim() != 1 or move1.shape[0] != B
                                  or move1.device != self.device or move1.stride(0) < 1):
            raise ValueError(f"move1 must be ({B},) int64 on the env's device")
        if out is None:
            out = t.empty((B, 9), dtype=t.int64, device=self.device)
        self.handle.call("narde_act_masks", _lib.ptr(d), _lib.ptr(move1),
                         move1.stride(0) if move1 is not None else 1, _lib.ptr(out), self._s())
        self._keep = (d, move1)
        return out

    def explore_plays(self, actions, epsilon, seed, tag, dice=None):
        """The DQN driver's exploration (narde_explore_plays): rows whose
        explore draw ({tag, row, 0, 5}, seed) is below epsilon get a play
        drawn uniformly from act()'s combination list written into their
        (B, 2) int64 action row (in place); epsilon (f32) and tag (int64)
        are device scalars (graph-safe)."""
        B, t = self.num_envs, self.torch
        if (actions.dtype != t.int64 or tuple(actions.shape) != (B, 2) or actions.stride(1) != 1
                or actions.device != self.device):
            raise ValueError(f"actions must be ({B}, 2) int64 rows on the env's device")
        d = None if dice is None else self._dev(dice, t.uint8, (B, 2))
        self.handle.call("narde_explore_plays", _lib.ptr(d), _lib.ptr(epsilon), int(seed) & (2 ** 64 - 1),
                         _lib.ptr(tag), _lib.ptr(actions), actions.stride(0), self._s())
        self._keep = (d,)
        return actions

    # ---------------------------------------- the checks the calls below share
    def _net_struct(self, net, none=""):
        """The check of a value net: its struct."""
        if not hasattr(net, "struct"):
            raise TypeError(f"net must be a gym_narde.value_net.ValueMLP{none}")
        mlp = net.struct()
        if net.l1.weight.device != self.device:
            raise ValueError("the net must live on the env's device")
        return mlp

    def _explore(self, epsilon, tag):
        """The explore pair as device scalars, (None, None) for greedy play."""
        t = self.torch
        if (epsilon is None) != (tag is None):
            raise ValueError("epsilon and tag go together")
        if epsilon is not None:
            epsilon = t.as_tensor(epsilon, dtype=t.float32, device=self.device).reshape(())
            tag = t.as_tensor(tag, dtype=t.int64, device=self.device).reshape(())
        return epsilon, tag

    def _check_records(self, a, text, least=1, most=None):
        """a is an (n, 8) int32 contiguous device tensor of records, least <=
        n (<= most), or a ValueError of the call's own text."""
        t = self.torch
        if (not isinstance(a, t.Tensor) or a.dtype != t.int32 or a.device != self.device or not a.is_contiguous()
                or a.dim() != 2 or a.shape[1] != 8 or a.shape[0] < least or (most is not None and a.shape[0] > most)):
            raise ValueError(text)

    def _row_values(self, aft, values):
        v, dim = values, values.dim()
        if dim == 2 and v.shape[1] == 1:
            v, dim = v[:, 0], 1
        n = v.shape[0] if dim == 1 else -1
        if (dim != 1 or v.dtype != self.torch.float32 or v.device != self.device or n < aft.cap
                or (n > 1 and v.stride(0) < 1)):
            raise ValueError(f"values must be float32, one per afterstate row (at least {aft.cap}), on the env's device")
        return v

    def _check_sel(self, sel):
        """sel is top_rows()' (B, k) int32 tensor: k."""
        t = self.torch
        if (not isinstance(sel, t.Tensor) or sel.dim() != 2 or sel.shape[0] != self.num_envs or sel.dtype != t.int32
                or not sel.is_contiguous() or sel.device != self.device):
            raise ValueError("sel must be top_rows()' (B, k) int32 tensor")
        return int(sel.shape[1])

    @staticmethod
    def _playout_sums(result, leaf):
        """(sums, trials, the leaf values or None) of a PlayoutResult or a
        (sums, trials[, leaf]) tuple, for a call with or without leaf."""
        if isinstance(result, PlayoutResult):
            sums, trials, lf = result.sums, result.trials, result.leaf
        else:
            sums, trials = result[0], int(result[1])
            lf = result[2] if len(result) > 2 else None
        if leaf and lf is None:
            raise ValueError("leaf=True needs the playouts' leaf values (playout(leaf=True))")
        return sums, trials, lf if leaf else None

    def _pick_out(self, k, slots=None):
        """New (actions, row[, score (B, slots)]) for a pick over rows of kind k."""
        t, B = self.torch, self.num_envs
        out = (t.empty((B,) + k.shape, dtype=getattr(t, k.dtype), device=self.device),
               t.empty(B, dtype=t.int32, device=self.device))
        return out if slots is None else out + (t.empty((B, slots), dtype=t.float32, device=self.device),)

    @staticmethod
    def _no_row(k, out):
        """A pick's outputs when no env has a row (cap == 0: no call, no array to read)."""
        for a, fill in zip(out, (k.no_row, -1, float("nan"))):
            a.fill_(fill)
        return tuple(out)

    def _turn_scratch(self, scratch, trials=None):
        """The FULL4 launches' scratch: the caller's, checked; or the env's
        own -- the rollouts', made once at min(B, resident waves) pieces, or
        with trials (a playout call's N * trials) the playouts'."""
        t = self.torch
        if scratch is not None:
            if (scratch.dtype != t.uint8 or scratch.device != self.device or not scratch.is_contiguous()
                    or scratch.numel() < _lib.turn_rollout_scratch_bytes(1)):
                raise ValueError("scratch must be a contiguous uint8 device tensor of at least one piece "
                                 f"({_lib.turn_rollout_scratch_bytes(1)} bytes; turn_value_rollout_scratch())")
            return scratch
        if trials is None:
            if getattr(self, "_turn_rollout_scratch", None) is None:
                self._turn_rollout_scratch = self.turn_value_rollout_scratch()
            return self._turn_rollout_scratch
        # min(N * trials, resident waves) pieces, kept on the env and grown when a call needs more
        # (the occupancy query is made once: a later call, inside a graph capture too, makes no other
        # call than the launch)
        if getattr(self, "_playout_waves", None) is None:
            self._playout_waves = self.turn_value_rollout_waves()
        need = _lib.turn_rollout_scratch_bytes(min(trials, self._playout_waves))
        if getattr(self, "_playout_scratch", None) is None or self._playout_scratch.numel() < need:
            self._playout_scratch = t.empty(need, dtype=t.uint8, device=self.device)
        return self._playout_scratch

    # ------------------------------------------------- the expansions' one core
    def _count_rows(self, k, d, offsets):
        """The counts alone (no array to write): the sizing call."""
        self.handle.call(k.expand, _lib.ptr(d), 0, _lib.ptr(offsets), None, None, None, None, None, self._s())

    def _new_rows(self, cap, shape, dtype):
        return self.torch.empty((cap,) + shape, dtype=dtype, device=self.device)

    def _row_cols(self, k, aft, offsets_required=False):
        """_rows()' columns every rows tuple has ahead of the call's own."""
        t = self.torch
        return (("offsets", aft.offsets, (self.num_envs + 1,), t.int32, offsets_required),
                ("row_env", aft.row_env, (), t.int32, False),
                (k.field, getattr(aft, k.field), k.shape, getattr(t, k.dtype), False))

    def _rows(self, k, dice, cap, aft, cols, text, feat=False, obs=False):
        """What every expansion of rows of kind k (a _RowKind) starts with:
        the dice; then either aft, a caller's tuple of preallocated arrays,
        checked -- cols: (name, tensor, trailing shape, dtype, required) of
        every array the call takes, offsets' shape whole; text: "out." or
        "out ", the call's wording --, or the sizing call when cap is None
        (the one synchronise) and a new tuple of cap rows.  Returns (dice,
        the tuple, cap)."""
        B, t = self.num_envs, self.torch
        d = None if dice is None else self._dev(dice, t.uint8, (B, 2))
        if aft is not None:
            cap = aft.cap if cap is None else int(cap)
            for name, a, shape, dt, required in cols:
                if a is None and not required:
                    continue
                ok = a is not None and a.dtype == dt and a.device == self.device and a.is_contiguous()
                ok = ok and (tuple(a.shape) == shape if name == "offsets" else
                             tuple(a.shape[1:]) == shape and a.shape[0] >= cap)
                if not ok:
                    raise ValueError(f"{text}{name} must be a contiguous {dt} device tensor of at least cap rows")
        else:
            offsets = t.empty(B + 1, dtype=t.int32, device=self.device)
            if cap is None:
                self._count_rows(k, d, offsets)
                cap = int(offsets[B].item())  # the one synchronise
            cap = int(cap)
            if cap < 0:
                raise ValueError("cap must be >= 0")
            aft = k.tuple(offsets, self._new_rows(cap, (), t.int32), self._new_rows(cap, k.shape, getattr(t, k.dtype)),
                          self._new_rows(cap, (198,), t.float32) if feat else None,
                          self._new_rows(cap, (24,), t.int32) if obs else None, self._new_rows(cap, (), t.int8), cap)
        if cap < 0:
            raise ValueError("cap must be >= 0")
        return d, aft, cap

    def _expand_rows(self, k, dice, cap, feat, obs, out):
        """afterstates() / turn_afterstates(): the rows of kind k."""
        t = self.torch
        cols = out and self._row_cols(k, out) + (("feat", out.feat, (198,), t.float32, False),
                                                 ("obs", out.obs, (24,), t.int32, False),
                                                 ("reward", out.reward, (), t.int8, False))
        d, out, cap = self._rows(k, dice, cap, out, cols, "out.", feat=feat, obs=obs)
        rows = (out.row_env, getattr(out, k.field), out.feat, out.obs, out.reward)
        self.handle.call(k.expand, _lib.ptr(d), cap, _lib.ptr(out.offsets),
                         *(_lib.ptr(a) if a is not None and cap > 0 else None for a in rows), self._s())
        self._keep = (d,)
        return out._replace(cap=cap)

    def _scored_rows(self, k, net, dice, cap, perspective, out, lookahead=False):
        """scored_afterstates() / scored_turn_afterstates(): the rows of kind
        k with their values under net in place of feat and obs.  lookahead:
        the two-ply values (lookahead_afterstates() / lookahead_turn_afterstates())."""
        if perspective not in PERSPECTIVES:
            raise ValueError(f"perspective must be one of {tuple(PERSPECTIVES)}")
        t = self.torch
        mlp = self._net_struct(net)
        values = cols = None
        if out is not None:
            if not hasattr(out, "offsets"):
                out, values = out
            cols = self._row_cols(k, out) + (("reward", out.reward, (), t.int8, False),
                                             ("values", values, (), t.float32, False))
        d, out, cap = self._rows(k, dice, cap, out, cols, "out ")
        if values is None:
            values = self._new_rows(cap, (), t.float32)
        if cap == 0:
            self._count_rows(k, d, out.offsets)
        else:
            args = (_lib.ptr(d), cap, _lib.ptr(out.offsets), _lib.ptr(out.row_env), _lib.ptr(getattr(out, k.field)),
                    _lib.ptr(out.reward), ctypes.byref(mlp), PERSPECTIVES[perspective], _lib.ptr(values))
            if lookahead:
                need = k.look_scratch(cap)
                if self._look_scratch is None or self._look_scratch.numel() < need:  # grown only when cap grows
                    self._look_scratch = t.empty(need, dtype=t.uint8, device=self.device)
                self.handle.call(k.expand + "_lookahead", *args, _lib.ptr(self._look_scratch),
                                 self._look_scratch.numel(), self._s())
            else:
                self.handle.call(k.expand + "_scored", *args, self._s())
        self._keep = (d, net)
        return out._replace(feat=None, obs=None, cap=cap), values[:cap]

    def scored_afterstates(self, net, dice=None, cap=None, perspective="white", out=None):
        """afterstates() with the rows scored on the way (narde_afterstates_scored;
        DESIGN.md section 15): net, a value_net.ValueMLP on the env's device, is
        evaluated inside the fill pass and one float a row is written -- the
        198-float rows are never made.  Returns (aft, values): aft an
        Afterstates with feat and obs None; values (cap,) float32 = net's
        value of each row, a terminal row's set to its outcome (reward, negated
        in perspective "white" when black made the move) -- what
        ValuePlayer.values() gives, ready for pick_afterstate().
        cap / out as afterstates(): cap None makes the one synchronise; cap
        given, or out = (an Afterstates of preallocated arrays, a (>= cap,)
        float32 values tensor) -- or the Afterstates alone, values then
        allocated --, none: graph-safe, and since the weights are
        read through pointers a replay sees net's weights of that moment
        (call net.pack() after changing them)."""
        if self.full:
            raise ValueError('scored_afterstates() is rules="ref2" only')
        return self._scored_rows(_REF2_ROWS, net, dice, cap, perspective, out)

    def lookahead_afterstates(self, net, dice=None, cap=None, out=None):
        """scored_afterstates() one ply deeper (narde_afterstates_lookahead;
        DESIGN.md section 17): the same rows, and for values white's two-ply
        value of each -- the mean, over the opponent's rolls in the env's dice
        mode, of the opponent's best reply under net (the smallest of the
        replies' one-ply values when black replies, the largest when white
        does; a roll with no reply takes the position step((0, 0)) leaves:
        the row's position with the mover flipped, include/narde.h has the one
        exception); a terminal row's is its outcome.  Returns (aft, values)
        shaped as scored_afterstates() returns them, the perspective "white";
        cap / out as there: cap None makes the one synchronise, cap or out
        given none (graph-safe).  The rows' records between the call's two
        passes live in a scratch tensor kept on the env, grown only when cap
        grows (so: outside capture, once, for the largest cap)."""
        if self.full:
            raise ValueError('lookahead_afterstates() is rules="ref2" only')
        return self._scored_rows(_REF2_ROWS, net, dice, cap, "white", out, lookahead=True)

    def scored_turn_afterstates(self, net, dice=None, cap=None, perspective="white", out=None):
        """rules="full4": scored_afterstates() over turn_afterstates()' rows
        (narde_turn_afterstates_scored, the overflow path included)."""
        if not self.full:
            raise ValueError('scored_turn_afterstates() is rules="full4" only')
        return self._scored_rows(_FULL4_ROWS, net, dice, cap, perspective, out)

    def lookahead_turn_afterstates(self, net, dice=None, cap=None, out=None):
        """rules="full4": scored_turn_afterstates() one ply deeper
        (narde_turn_afterstates_lookahead): the same
        rows, and for values white's two-ply value of each -- the mean, over
        the opponent's rolls in the env's dice mode (the unordered rolls, a
        double once and any other twice), of the opponent's best whole-turn
        reply under net (the smallest of the replies' one-ply values when
        black replies, the largest when white does; a roll with no legal
        sub-move takes the row's position with the mover flipped); a terminal
        row's is its outcome.  Every reply set is exact, the overflow paths
        included.  Returns (aft, values) shaped as scored_turn_afterstates()
        returns them, the perspective "white"; cap / out and the scratch
        tensor as lookahead_afterstates()."""
        if not self.full:
            raise ValueError('lookahead_turn_afterstates() is rules="full4" only')
        return self._scored_rows(_FULL4_ROWS, net, dice, cap, "white", out, lookahead=True)

    def _recorded_rows(self, k, net, dice, cap, out):
        """recorded_afterstates() / recorded_turn_afterstates(): the rows of
        kind k with their records, and their values when net is given."""
        t = self.torch
        mlp = None if net is None else self._net_struct(net, none=" or None")
        aft = values = records = cols = None
        if out is not None:
            aft, values, records = out
            if (aft.cap if cap is None else int(cap)) < 0:  # (this call looks at cap before its arrays)
                raise ValueError("cap must be >= 0")
            cols = self._row_cols(k, aft, True) + (("reward", aft.reward, (), t.int8, False),
                                                   ("values", values, (), t.float32, net is not None),
                                                   ("records", records, (8,), t.int32, True))
        d, aft, cap = self._rows(k, dice, cap, aft, cols, "out ")
        if out is None:
            values = self._new_rows(cap, (), t.float32) if net is not None else None
            records = self._new_rows(cap, (8,), t.int32)
        if cap == 0:
            self._count_rows(k, d, aft.offsets)
        else:
            self.handle.call(k.expand + "_records", _lib.ptr(d), cap, _lib.ptr(aft.offsets), _lib.ptr(aft.row_env),
                             _lib.ptr(getattr(aft, k.field)), _lib.ptr(aft.reward),
                             ctypes.byref(mlp) if mlp is not None else None, PERSPECTIVES["white"],
                             _lib.ptr(values) if net is not None else None, _lib.ptr(records), self._s())
        self._keep = (d, net, mlp)
        return (aft._replace(feat=None, obs=None, cap=cap), (values[:cap] if net is not None else None),
                records[:cap])

    def recorded_afterstates(self, net, dice=None, cap=None, out=None):
        """scored_afterstates() (perspective "white") with each row's record
        as a third output (narde_afterstates_records):
        returns (aft, values, records), records (cap, 8) int32 = the 32-byte
        record step(aft.codes[r], autoreset off) leaves in env aft.row_env[r],
        its ply counter included -- a playout() root as it stands.  net None:
        the records alone, values None.  cap / out as scored_afterstates():
        cap None makes the one synchronise; cap given, or out = (an
        Afterstates, a (>= cap,) float32 values tensor or None, a (>= cap, 8)
        int32 records tensor), none (graph-safe)."""
        if self.full:
            raise ValueError('recorded_afterstates() is rules="ref2" only')
        return self._recorded_rows(_REF2_ROWS, net, dice, cap, out)

    def recorded_turn_afterstates(self, net, dice=None, cap=None, out=None):
        """rules="full4": recorded_afterstates() over turn_afterstates()' rows
        (narde_turn_afterstates_records, the overflow path included)."""
        if not self.full:
            raise ValueError('recorded_turn_afterstates() is rules="full4" only')
        return self._recorded_rows(_FULL4_ROWS, net, dice, cap, out)

    def top_rows(self, aft, values, k, records=None, perspective="white", out=None):
        """Each env's k best rows of `aft` by `values`, best first
        (narde_rows_topk), under exactly
        pick_afterstate()'s / pick_turn()'s greedy order -- perspective, ties to
        the lowest row, NaNs first --, so sel[:, 0] is the row those return.
        Returns (sel (B, k) int32, -1 behind an env's last row; roots (B * k, 8)
        int32 = records[sel] -- the none record, an empty board with both
        sides' 15 checkers off, in an empty slot -- or None without records).
        out: (sel, roots or None) of an earlier call to write into.  Call it
        before the step (it reads who moves).  No synchronise."""
        if perspective not in PERSPECTIVES:
            raise ValueError(f"perspective must be one of {tuple(PERSPECTIVES)}")
        B, t, k = self.num_envs, self.torch, int(k)
        if not 1 <= k <= _lib.TOPK_MAX:
            raise ValueError(f"k must be in 1 .. {_lib.TOPK_MAX}")
        v = self._row_values(aft, values)
        if records is not None:
            self._check_records(records, "records must be a contiguous (>= cap, 8) int32 device tensor", aft.cap)
        if out is not None:
            sel, roots = out
        else:
            sel = t.empty((B, k), dtype=t.int32, device=self.device)
            roots = t.empty((B * k, 8), dtype=t.int32, device=self.device) if records is not None else None
        if aft.cap == 0:  # no row anywhere (and no array to read)
            sel.fill_(-1)
            if roots is not None:
                roots.zero_()
                roots[:, 6] = _lib.RECORD_NONE_WORD6
            return sel, roots
        self.handle.call("narde_rows_topk", _lib.ptr(aft.offsets), aft.cap, _lib.ptr(v), max(1, v.stride(0)),
                         PERSPECTIVES[perspective], k, _lib.ptr(records), _lib.ptr(sel), _lib.ptr(roots), self._s())
        self._keep = (v, records)
        return sel, roots

    def pick_playout(self, aft, values, sel, result, leaf=False, out=None):
        """The playout-greedy move (narde_playout_pick / narde_turn_playout_pick
        by the env's rules): per env the candidate of
        sel (top_rows()') with the best playout score.  values: white's
        one-ply values of aft's rows (a perspective "white" call); result: the
        PlayoutResult of playout() over top_rows()' roots, or a (sums, trials[,
        leaf]) tuple.  A slot's score: a terminal row's outcome; else the mean
        outcome of its finished trials (the one-ply value when none
        finished), or with leaf=True the truncated mean (points + the
        unfinished trials' leaves) / trials.  The largest when white moves,
        the smallest when black does, the lowest slot on ties.  Returns
        (actions (B,2) int16 or play (B,4,2) int8 for step(), row (B,) int32,
        score (B, k) float32 -- NaN where a slot is empty); -1 and (0, 0) / an
        all -1 play for an env with no candidate.  out: an earlier call's
        triple to write into.  Call it before the step.  No synchronise."""
        t, B, kind = self.torch, self.num_envs, self._kind
        sums, trials, lf = self._playout_sums(result, leaf)
        k = self._check_sel(sel)
        if (tuple(sums.shape) != (B * k, 4) or sums.dtype != t.int32 or not sums.is_contiguous()
                or sums.device != self.device):
            raise ValueError("result must hold the sums of B * k roots")
        if lf is not None and (tuple(lf.shape) != (B * k, trials) or lf.dtype != t.float32 or not lf.is_contiguous()):
            raise ValueError("leaf must be (B * k, trials) float32")
        v = self._row_values(aft, values)
        if out is None:
            out = self._pick_out(kind, k)
        if aft.cap == 0:
            return self._no_row(kind, out)
        actions, row, score = out
        self.handle.call(kind.playout_pick, k, _lib.ptr(sel), aft.cap, _lib.ptr(v), max(1, v.stride(0)),
                         _lib.ptr(aft.reward), _lib.ptr(getattr(aft, kind.field)), trials, _lib.ptr(sums), _lib.ptr(lf),
                         _lib.ptr(actions), _lib.ptr(row), _lib.ptr(score), self._s())
        self._keep = (v, sel, sums, lf)
        return actions, row, score

    def lookahead_records(self, records, net, out=None):
        """White's two-ply value of given positions (narde_records_lookahead /
        narde_turn_records_lookahead by the env's rules):
        what lookahead_afterstates() / lookahead_turn_afterstates() give a row,
        for any records -- top_rows()' roots, a records rollout's
        bufs["records"], state_records().  records: an (n, 8) int32 device
        tensor; its ply-counter word and elapsed are ignored.  Returns an (n,)
        float32 tensor: the mean, over the rolls of the record's mover in the
        env's dice mode, of the mover's best afterstate under net (the
        smallest one-ply value for black, the largest for white; terminal
        replies at their outcome); NaN for a record whose game is over (either
        side has 15 off: a finished game, top_rows()' none record).  On the
        records of a roll's rows the values are the full searches' bit for
        bit.  This env's positions, ply counter and statistics are neither
        read nor written.  out: an (n,) float32 tensor to write into.
        rules="full4": the call's 128-byte row pieces live in a scratch tensor
        kept on the env and grown when a later call has more records -- a
        caller capturing a graph makes its first call outside capture, with its
        largest n.  No synchronise."""
        t, kind = self.torch, self._kind
        self._check_records(records, "records must be a contiguous (n, 8) int32 device tensor of records, n >= 1")
        mlp = self._net_struct(net)
        n = int(records.shape[0])
        if out is None:
            out = t.empty(n, dtype=t.float32, device=self.device)
        elif (tuple(out.shape) != (n,) or out.dtype != t.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError("out must be a contiguous (n,) float32 device tensor")
        scratch, tail = None, ()
        if kind.turn_scratch:
            need = kind.look_scratch(n)
            if getattr(self, "_records_look_scratch", None) is None or self._records_look_scratch.numel() < need:
                self._records_look_scratch = t.empty(need, dtype=t.uint8, device=self.device)
            scratch = self._records_look_scratch
            tail = (_lib.ptr(scratch), int(scratch.numel()))
        self.handle.call(kind.records_lookahead, n, _lib.ptr(records), ctypes.byref(mlp), _lib.ptr(out), *tail,
                         self._s())
        self._keep = (records, net, mlp, out, scratch)
        return out

    def pick_slots(self, aft, values, sel, slot_score, out=None):
        """The move by given scores of top_rows()' candidates (narde_slot_pick /
        narde_turn_slot_pick by the env's rules):
        pick_playout() with slot_score (B, k) float32 -- white's score of each
        slot, e.g. lookahead_records() of top_rows()' roots reshaped -- in
        place of the playouts.  A slot's score: a terminal row's outcome
        (values[row]); else slot_score; an empty slot's is NaN and never
        picked.  The largest when white moves, the smallest when black does,
        the lowest slot on ties, NaN as the picks take it.  Returns (actions
        (B,2) int16 or play (B,4,2) int8 for step(), row (B,) int32, score
        (B, k) float32); -1 and (0, 0) / an all -1 play for an env with no
        candidate.  out: an earlier call's triple to write into.  Call it
        before the step.  No synchronise."""
        t, B, kind = self.torch, self.num_envs, self._kind
        k = self._check_sel(sel)
        if not 1 <= k <= _lib.TOPK_MAX:
            raise ValueError(f"k must be in 1 .. {_lib.TOPK_MAX}")
        if (not isinstance(slot_score, t.Tensor) or slot_score.dtype != t.float32 or slot_score.device != self.device
                or not slot_score.is_contiguous() or slot_score.numel() != B * k
                or tuple(slot_score.shape) not in ((B, k), (B * k,))):
            raise ValueError("slot_score must be a contiguous (B, k) or (B * k,) float32 device tensor")
        v = self._row_values(aft, values)
        if out is None:
            out = self._pick_out(kind, k)
        if aft.cap == 0:
            return self._no_row(kind, out)
        actions, row, score = out
        self.handle.call(kind.slot_pick, k, _lib.ptr(sel), aft.cap, _lib.ptr(v), max(1, v.stride(0)),
                         _lib.ptr(aft.reward), _lib.ptr(getattr(aft, kind.field)), _lib.ptr(slot_score),
                         _lib.ptr(actions), _lib.ptr(row), _lib.ptr(score), self._s())
        self._keep = (v, sel, slot_score)
        return actions, row, score

    def _pick_rows(self, k, aft, values, perspective, epsilon, tag, seed):
        """pick_afterstate() / pick_turn(): the row's action, k.no_row for none."""
        if perspective not in PERSPECTIVES:
            raise ValueError(f"perspective must be one of {tuple(PERSPECTIVES)}")
        v = self._row_values(aft, values)
        if epsilon is not None or tag is not None:
            epsilon, tag = self._explore(epsilon, tag)
        out = actions, row = self._pick_out(k)
        if aft.cap == 0:
            return self._no_row(k, out)
        self.handle.call(k.pick, _lib.ptr(aft.offsets), _lib.ptr(getattr(aft, k.field)), aft.cap, _lib.ptr(v),
                         max(1, v.stride(0)), PERSPECTIVES[perspective], _lib.ptr(epsilon), int(seed) & (2 ** 64 - 1),
                         _lib.ptr(tag), _lib.ptr(actions), _lib.ptr(row), self._s())
        self._keep = (v, epsilon, tag)
        return out

    def afterstates(self, dice=None, cap=None, feat=True, obs=False, out=None):
        """The successor positions of each env's roll (narde_afterstates; what
        a TD-Gammon value network scores, README.md:42-102), for dice (B,2) in
        roll order or the next step's device dice: per env the plays
        NardeEnv.step carries out (narde_env.py:27-103) in list order, less
        those action codes cannot express, the first of those that leave the
        same board and off counts kept.  Returns Afterstates(offsets (B+1,)
        int32, row_env (R,) int32, codes (R,2) int16 -- feed them to step()
        --, feat (R,198) float32 = tesauro198() after that step, obs (R,24)
        int32 or None, reward (R,) int8 -- 0, or 1 / 2 at a terminal
        afterstate --, cap = R).
        cap None: a count pass, then offsets[B] is read on the host -- the
        call's ONE synchronise -- and the arrays are allocated exactly.  cap
        given (or out: an Afterstates of preallocated arrays, cap rows of
        them used): one stream-ordered call with no synchronise, safe to
        capture in a graph; rows from cap on are not written, and offsets
        still holds the true counts."""
        if self.full:
            raise ValueError('afterstates() is rules="ref2" only')
        return self._expand_rows(_REF2_ROWS, dice, cap, feat, obs, out)

    def pick_afterstate(self, aft, values, perspective="white", epsilon=None, tag=None, seed=0):
        """Value-greedy play (narde_afterstate_pick): per env the row of `aft`
        with the best of values (one float32 per row of aft.feat: (R,) or
        (R,1), any row stride) -- perspective "mover": the largest;
        "white" (the README's reward, +1 if WHITE wins): the largest when
        white moves, the smallest when black does; the lowest row on ties.
        epsilon (f32) / tag (int64) device scalars (or numbers): the env's
        explore draw ({tag, env, 0, 5}, seed) below epsilon takes a uniform
        row instead.  Call it before the step (it reads who moves).
        Returns (actions (B,2) int16 for step(), row (B,) int32; -1 and
        (0, 0) for an env with no row)."""
        return self._pick_rows(_REF2_ROWS, aft, values, perspective, epsilon, tag, seed)

    def turn_afterstates(self, dice=None, cap=None, feat=True, obs=False, out=None):
        """rules="full4": the distinct positions each env's whole turn can
        leave (narde_turn_afterstates; four sub-moves on doubles, the
        max-dice-used rule), for dice (B,2) or the next step's device dice.
        Rows are ordered by the first play -- plays in lexicographic order,
        sub-moves in list order: higher die first, source ascending -- that
        produces each one; a pass or a die outside 1..6 gives no row.
        Returns TurnAfterstates(offsets (B+1,) int32, row_env (R,) int32,
        play (R,4,2) int8 (from, die), -1 padded -- feed them to step() --,
        feat (R,198) float32 = tesauro198() after that turn, obs (R,24)
        int32 or None, reward (R,) int8 -- 0, or 1 / 2 at a terminal
        afterstate --, cap = R).  cap / out as afterstates(): cap None runs
        the count pass and reads offsets[B] on the host -- the call's ONE
        synchronise; cap given (or out) is one stream-ordered call, safe to
        capture in a graph once the handle has made one call outside
        capture (its workspace is allocated then)."""
        if not self.full:
            raise ValueError('turn_afterstates() is rules="full4" only')
        return self._expand_rows(_FULL4_ROWS, dice, cap, feat, obs, out)

    def pick_turn(self, aft, values, perspective="white", epsilon=None, tag=None, seed=0):
        """pick_afterstate() over turn_afterstates' rows (narde_turn_pick: the
        same perspective, tie, NaN and explore-draw rules).  Returns (play
        (B,4,2) int8 for step(), row (B,) int32; -1 and an all -1 play for
        an env with no row)."""
        if not self.full:
            raise ValueError('pick_turn() is rules="full4" only')
        return self._pick_rows(_FULL4_ROWS, aft, values, perspective, epsilon, tag, seed)

    def legal_full(self, dice=None):
        """FULL4: (B,) int64 legal words (first sub-move set | max dice << 56)
        for dice (B,2) or the next step's device dice."""
        B = self.num_envs
        d = None if dice is None else self._dev(dice, self.torch.uint8, (B, 2))
        out = self.torch.empty(B, dtype=self.torch.int64, device=self.device)
        self.handle.call("narde_legal_full", _lib.ptr(d), _lib.ptr(out), self._s())
        return out

    def step(self, actions=None, dice=None):
        """NardeEnv.step for all envs.  actions (B,2) codes (rules="full4":
        (B,4,2) int8 (from, die) plays) or None for the in-kernel random
        legal policy; dice (B,2) or None for device dice.  Returns (obs,
        reward, terminated, truncated, info) device tensors; info =
        {'legal': compact list #1, 'actions': codes used} (rules="full4":
        {'legal': first sub-move set + max dice, 'played': sub-moves})."""
        B = self.num_envs
        if self.full:
            a = None if actions is None else self._dev(actions, self.torch.int8, (B, 4, 2))
        else:
            a = None if actions is None else self._dev(actions, self.torch.int16, (B, 2))
        d = None if dice is None else self._dev(dice, self.torch.uint8, (B, 2))
        rc = self._step_fn(self.handle.h, None if a is None else _lib.ptr(a), None if d is None else _lib.ptr(d),
                           *self._step_out, int(self.autoreset), self._s())
        if rc:
            _lib.check(rc, self._kind.step)
        if self.full:
            self._keep = (a, d)
            return (self.obs, self.reward, self.terminated, self.truncated,
                    {"legal": self.legal, "played": self.played})
        return (self.obs, self.reward, self.terminated, self.truncated,
                {"legal": self.legal, "actions": self.actions_used})

    def selfplay(self, plies):
        """plies plies of random-legal self-play in ONE launch (statistics only)."""
        self.handle.call(self._kind.selfplay, int(plies), self._s())

    def rollout_buffers(self, plies, obs=True, reward=True, terminated=True, truncated=True,
                        legal=True, actions=True):
        """Allocate [plies][B] rollout buffers for rollout() (rules="full4":
        'actions' holds the played sub-moves, (plies, B) int64)."""
        t, B, dev = self.torch, self.num_envs, self.device
        mk = lambda on, shape, dt: t.empty(shape, dtype=dt, device=dev) if on else None  # noqa: E731
        act = mk(actions, (plies, B), t.int64) if self.full else mk(actions, (plies, B, 2), t.int16)
        return dict(obs=mk(obs, (plies, B, 24), t.int32), reward=mk(reward, (plies, B), t.int32),
                    terminated=mk(terminated, (plies, B), t.uint8),
                    truncated=mk(truncated, (plies, B), t.uint8),
                    legal=mk(legal, (plies, B), t.int64), actions=act)

    def rollout(self, plies, bufs=None):
        """plies plies of random-legal self-play (auto-reset) in ONE launch,
        every ply's outputs streamed into [plies][B] buffers (see
        rollout_buffers); equals `plies` calls of step()."""
        if bufs is None:
            bufs = self.rollout_buffers(plies)
        for v in bufs.values():
            if v is not None and v.shape[0] < plies:
                raise ValueError("rollout buffer shorter than plies")
        self.handle.call(self._kind.rollout, int(plies),
                         _lib.ptr(bufs["obs"]), _lib.ptr(bufs["reward"]),
                         _lib.ptr(bufs["terminated"]), _lib.ptr(bufs["truncated"]),
                         _lib.ptr(bufs["legal"]), _lib.ptr(bufs["actions"]), self._s())
        return bufs

    def value_rollout_buffers(self, plies, dice=True, actions=True, value=True, reward=True, terminated=True,
                              truncated=True, records=False):
        """Allocate value_rollout()'s [plies][B] buffers: dice (plies,B,2)
        uint8, actions (plies,B,2) int16, value (plies,B) float32, reward
        (plies,B) int32, terminated / truncated (plies,B) uint8; None for
        one switched off.  records (off by default): (plies,B,8) int32, each
        env's 32-byte record as the ply found it (what
        td.WindowTDLambdaLearner trains on)."""
        return self._rollout_buffers(_REF2_ROWS, plies, (dice, actions, value, reward, terminated, truncated), records)

    def _rollout_buffers(self, k, plies, on, records=False):
        """k.bufs as [plies][B] tensors, None where `on` switches one off."""
        t, B, plies = self.torch, self.num_envs, int(plies)
        bufs = {name: t.empty((plies, B) + shape, dtype=getattr(t, dt), device=self.device) if flag else None
                for (name, shape, dt), flag in zip(k.bufs, on)}
        if records:  # (the key exists only then: callers walk the dict)
            bufs["records"] = t.empty((plies, B, 8), dtype=t.int32, device=self.device)
        return bufs

    def _net_pair(self, net_white, net_black):
        """A launch's net per colour, checked: (net_white, net_black, their
        structs -- None for a colour that plays the random-legal policy)."""
        if net_black is _SAME:
            net_black = net_white
        if net_white is None and net_black is None:
            raise ValueError("a net for at least one colour (random play on both sides is selfplay())")
        white = None if net_white is None else self._net_struct(net_white)
        black = white if net_black is net_white else None if net_black is None else self._net_struct(net_black)
        return net_white, net_black, [white, black]  # (one struct serves both colours of one net)

    def _value_rollout(self, entry, plies, who, epsilon, tag, seed, bufs, scratch, league=False):
        """The one launch body of value_rollout(), turn_value_rollout() and
        their league twins, by the env's rule set: the checks in their order
        -- plies, who plays (net_white, net_black; a league's table, white,
        black), the explore pair, the buffers, the scratch -- and the call."""
        k, plies = self._kind, int(plies)
        if plies < 1:
            raise ValueError("plies must be >= 1")
        if league:
            table, white, black = who
            head = (_lib.ptr(table), self._league_args(table, white, black), _lib.ptr(white), _lib.ptr(black))
        else:
            who = _, _, (mw, mb) = self._net_pair(*who)
            head = (None if mw is None else ctypes.byref(mw), None if mb is None else ctypes.byref(mb))
        if epsilon is not None or tag is not None:
            epsilon, tag = self._explore(epsilon, tag)
        if bufs is None:
            bufs = self._rollout_buffers(k, plies, (True,) * len(k.bufs))
        ptrs = []  # the buffers' pointers in the launch's order, the records' last
        for name, dtype, shape, dt in self._buf_specs:
            a = bufs.get(name)
            if a is not None and (a.dtype != dtype or a.device != self.device or not a.is_contiguous() or a.dim() < 2
                                  or a.shape[0] < plies or tuple(a.shape[1:]) != shape):
                raise ValueError(f"bufs[{name!r}] must be a contiguous {dt} device tensor of shape "
                                 f"(>= {plies}{''.join(f', {n}' for n in shape)})")
            ptrs.append(_lib.ptr(a))
        tail = keep = ()
        if k.turn_scratch:
            scratch = self._turn_scratch(scratch)
            tail, keep = (_lib.ptr(scratch), int(scratch.numel())), (scratch,)
        self.handle.call(entry, plies, *head, _lib.ptr(epsilon), int(seed) & (2 ** 64 - 1), _lib.ptr(tag),
                         *ptrs[:-1], *tail, ptrs[-1], self._s())
        self._keep = who + (epsilon, tag, bufs) + keep
        return bufs

    def value_rollout(self, plies, net_white, net_black=_SAME, epsilon=None, tag=None, seed=0, bufs=None):
        """plies plies of value-greedy play in ONE launch, a net per colour
        (narde_value_rollout): every ply is what
        ValuePlayer.step() does on its fused path -- the next step's dice,
        scored_afterstates() under the mover's net (perspective "white"),
        pick_afterstate(epsilon, tag + k, seed) for ply k, step() with
        auto-reset -- with no row or value written on the way.  net_white /
        net_black: value_net.ValueMLPs on the env's device (net_black
        defaults to net_white); None for one colour makes that colour play
        the random-legal policy, bit for bit step()'s own.  epsilon (f32) /
        tag (int64): device scalars or numbers, together or not at all.
        Returns bufs (value_rollout_buffers(): made when not given; an entry
        None is not written): dice, actions, value -- white's value of the row
        played, NaN on a random ply and where there was no row --, reward,
        terminated, truncated, each [plies][B]; and, where bufs has it,
        records (value_rollout_buffers(records=True)).  Statistics and the ply
        counter advance as in step().  No synchronise; graph-safe when bufs,
        epsilon and tag are given as device tensors (the weights are read
        through pointers: call net.pack() after changing them)."""
        if self.full:
            raise ValueError('value_rollout() is rules="ref2" only')
        return self._value_rollout(self._kind.value_rollout, plies, (net_white, net_black), epsilon, tag, seed, bufs,
                                   None)

    def turn_value_rollout_buffers(self, plies, dice=True, play=True, value=True, reward=True, terminated=True,
                                   truncated=True, records=False):
        """Allocate turn_value_rollout()'s [plies][B] buffers:
        value_rollout_buffers() with play (plies,B,4,2) int8 -- the (from,
        die) sub-moves, -1 padded -- in place of actions."""
        return self._rollout_buffers(_FULL4_ROWS, plies, (dice, play, value, reward, terminated, truncated), records)

    def turn_value_rollout_waves(self):
        """The waves the device keeps resident for turn_value_rollout()'s
        kernel (narde_turn_value_rollout_waves; launches nothing)."""
        w = ctypes.c_int(0)
        self.handle.call("narde_turn_value_rollout_waves", ctypes.byref(w))
        return w.value

    def turn_value_rollout_scratch(self, waves=None):
        """A scratch tensor for turn_value_rollout(): `waves` pieces
        (default min(B, turn_value_rollout_waves())), uint8 on the env's
        device."""
        if waves is None:
            waves = min(self.num_envs, self.turn_value_rollout_waves())
        if int(waves) < 1:
            raise ValueError("waves must be >= 1")
        return self.torch.empty(_lib.turn_rollout_scratch_bytes(waves), dtype=self.torch.uint8, device=self.device)

    def turn_value_rollout(self, plies, net_white, net_black=_SAME, epsilon=None, tag=None, seed=0, bufs=None,
                           scratch=None):
        """rules="full4": value_rollout() over whole turns
        (narde_turn_value_rollout).  Every ply is what
        ValuePlayer.step() does on a FULL4 env -- the next step's dice,
        scored_turn_afterstates() under the mover's net (perspective
        "white"), pick_turn(epsilon, tag + k, seed) for ply k, step() with
        that play and auto-reset -- with no row or value written on the way;
        an env with no row passes.  The nets, epsilon, tag and seed are
        value_rollout()'s; a colour with None plays the random-legal policy,
        bit for bit step()'s own.
        Returns bufs (turn_value_rollout_buffers(): made when not given; an
        entry None is not written): dice, play (plies,B,4,2) int8, value --
        white's value of the row played, NaN on a random ply and on a pass --,
        reward, terminated, truncated; and, where bufs has it, records
        (turn_value_rollout_buffers(records=True)).
        scratch: a uint8 device tensor of whole pieces
        (turn_value_rollout_scratch()); the launch has as many one-wave
        workgroups as it has pieces, B at most, and gives the same bits
        whatever their number.  Not given: allocated once at min(B, resident
        waves) pieces and kept on the env -- a caller capturing a graph makes
        its first call outside capture or passes its own.  No synchronise;
        graph-safe when bufs, scratch, epsilon and tag are given as device
        tensors."""
        if not self.full:
            raise ValueError('turn_value_rollout() is rules="full4" only')
        return self._value_rollout(self._kind.value_rollout, plies, (net_white, net_black), epsilon, tag, seed, bufs,
                                   scratch)

    def net_table(self, nets, out=None):
        """The league launches' table of 1 .. 64 value_net.ValueMLPs on the
        env's device (narde_net_table): a uint8 device
        tensor of 64 bytes a net, written on the current stream by small
        launches that carry the nets in their arguments -- no host copy, no
        synchronise, graph-safe when out is given.  The table holds pointers,
        not weights: after the weights change call net.pack(), as for every
        other call, and the next launch sees them.  out: a contiguous uint8
        device tensor of at least that size, 16-B aligned (the table is its
        first 64 x len(nets) bytes, returned as a view).  The env keeps the
        nets alive for as long as it lives."""
        t = self.torch
        nets = list(nets)
        if not 1 <= len(nets) <= _lib.LEAGUE_NETS_MAX:
            raise ValueError(f"a table holds 1 .. {_lib.LEAGUE_NETS_MAX} nets, not {len(nets)}")
        structs = (_lib.ValueMlp * len(nets))()
        for i, net in enumerate(nets):
            if not hasattr(net, "struct"):  # (the table's own wording, the device before the struct)
                raise TypeError(f"nets[{i}] must be a gym_narde.value_net.ValueMLP")
            if net.l1.weight.device != self.device:
                raise ValueError(f"nets[{i}] must live on the env's device")
            structs[i] = net.struct()
        nbytes = _lib.league_table_bytes(len(nets))
        if out is None:
            out = t.empty(nbytes, dtype=t.uint8, device=self.device)
        elif (out.dtype != t.uint8 or out.device != self.device or not out.is_contiguous() or out.dim() != 1
              or out.numel() < nbytes or out.data_ptr() % 16):
            raise ValueError(f"out must be a contiguous, 16-B aligned uint8 device tensor of at least {nbytes} bytes")
        table = out[:nbytes]
        _lib.check(self.handle.lib.narde_net_table(self.device.index, len(nets), structs, _lib.ptr(table), nbytes,
                                                   self._s()), "narde_net_table")
        if getattr(self, "_league_nets", None) is None:
            self._league_nets = {}
        self._league_nets[table.data_ptr()] = tuple(nets)
        return table

    def _league_args(self, table, white, black):
        """The league launches' checks of the table and the two index
        tensors: the number of nets."""
        t, B, entry = self.torch, self.num_envs, _lib.league_table_bytes(1)
        if (not isinstance(table, t.Tensor) or table.dtype != t.uint8 or table.device != self.device
                or not table.is_contiguous() or table.dim() != 1 or table.numel() % entry
                or not 1 <= table.numel() // entry <= _lib.LEAGUE_NETS_MAX or table.data_ptr() % 16):
            raise ValueError("table must be net_table()'s uint8 tensor on the env's device")
        for name, a in (("white", white), ("black", black)):
            if (not isinstance(a, t.Tensor) or a.dtype != t.int32 or a.device != self.device or not a.is_contiguous()
                    or tuple(a.shape) != (B,)):
                raise ValueError(f"{name} must be a contiguous int32 device tensor of shape ({B},)")
        return table.numel() // entry

    def value_rollout_league(self, plies, table, white, black, epsilon=None, tag=None, seed=0, bufs=None):
        """value_rollout() with a net per env and colour
        (narde_value_rollout_league): env e's white
        plies are played under net white[e] of table (net_table()), its black
        plies under net black[e], through every game the env plays inside the
        launch.  white, black: (B,) int32 device tensors, read on the device;
        an index outside the table (-1, say) makes that colour of that env
        play the random-legal policy, bit for bit step()'s own; both colours
        random, and white[e] == black[e], are allowed.  Env e's outputs,
        state and stats() are bit for bit value_rollout()'s under those two
        nets.  plies, epsilon, tag, seed, bufs (value_rollout_buffers(),
        records=True included) and the return value are value_rollout()'s.
        No synchronise; graph-safe under value_rollout()'s conditions, with
        white and black rewritten in place between replays."""
        if self.full:
            raise ValueError('value_rollout_league() is rules="ref2" only')
        return self._value_rollout(self._kind.league, plies, (table, white, black), epsilon, tag, seed, bufs, None,
                                   league=True)

    def turn_value_rollout_league(self, plies, table, white, black, epsilon=None, tag=None, seed=0, bufs=None,
                                  scratch=None):
        """rules="full4": turn_value_rollout() with value_rollout_league()'s
        table, white and black (narde_turn_value_rollout_league).  bufs
        (turn_value_rollout_buffers()) and scratch are turn_value_rollout()'s:
        the same bits whatever the number of pieces."""
        if not self.full:
            raise ValueError('turn_value_rollout_league() is rules="full4" only')
        return self._value_rollout(self._kind.league, plies, (table, white, black), epsilon, tag, seed, bufs, scratch,
                                   league=True)

    def state_records(self, board, off, first_turn, player, t=0):
        """N positions (set_state()'s arrays, any N) as the 32-byte records
        the records rollouts write: an (N, 8) int32 device tensor, the ply
        counter t, elapsed 0 (narde_state_records).  What playout() takes as
        roots and td.WindowTDLambdaLearner as records."""
        tt = self.torch
        b = tt.as_tensor(board, device=self.device).to(tt.int8).contiguous()
        if b.dim() != 2 or b.shape[1] != 24 or b.shape[0] < 1:
            raise ValueError(f"board must be (N, 24) with N >= 1, got {tuple(b.shape)}")
        N = int(b.shape[0])
        o = self._dev(off, tt.uint8, (N, 2))
        f = self._dev(first_turn, tt.uint8, (N, 2))
        p = self._dev(player, tt.int8, (N,))
        rec = tt.empty((N, 8), dtype=tt.int32, device=self.device)
        _lib.check(self.handle.lib.narde_state_records(self.device.index, N, _lib.ptr(b), _lib.ptr(o), _lib.ptr(f),
                                                       _lib.ptr(p), int(t) & 0xFFFFFFFF, _lib.ptr(rec), self._s()),
                   "narde_state_records")
        self._keep = (b, o, f, p)
        return rec

    def playout(self, roots, trials, net_white, net_black=_SAME, max_plies=1000, seed=0, id_base=0,
                common_dice=False, per_trial=False, leaf=False, scratch=None, out=None):
        """Monte-Carlo playouts (narde_value_playout / narde_turn_value_playout
        by the env's rules): every root position played
        `trials` times to the end -- max_plies plies at most -- both colours
        value-greedy under their nets (None: that colour plays the
        random-legal policy), each trial on a dice stream of its own.  roots:
        an (N, 8) int32 device tensor of records (state_records(), or a
        records rollout's bufs["records"][k]) or a get_state()-style dict,
        packed with state_records() at ply counter 0.  Trial j of root i plays
        what value_rollout() / turn_value_rollout() plays at env index
        i * trials + j of an env made with `seed`, env_id_offset=id_base, this
        env's dice mode and max_episode_steps=0, up to its first terminal ply;
        common_dice: index j for every root, so that all roots see the same
        dice in trial j.  This env's own positions, ply counter and
        statistics are neither read nor written.
        Returns a PlayoutResult: finished, points, squares, plies -- (N,)
        int32 views of its sums --, and with per_trial outcome (N, trials)
        int8 and length (N, trials) int32, with leaf the (N, trials) float32
        leaf values of the unfinished trials (NaN where finished).  out: an
        earlier result of the same shape to write into (no allocation: graph
        capture).  scratch (full4): as turn_value_rollout()'s; not given, it is
        allocated at min(N * trials, resident waves) pieces, kept on the env
        and grown when a later call needs more -- a caller capturing a graph
        makes its first call outside capture or passes its own.  The same
        inputs give the same bits whatever its size.  No synchronise."""
        t = self.torch
        if isinstance(roots, dict):
            roots = self.state_records(roots["board"], roots["off"], roots["first_turn"], roots["player"])
        self._check_records(roots, "roots must be a contiguous (N, 8) int32 device tensor of records, or a get_state() "
                                   "dict")
        N, trials, max_plies = int(roots.shape[0]), int(trials), int(max_plies)
        if trials < 1 or max_plies < 1:
            raise ValueError("trials and max_plies must be >= 1")
        net_white, net_black, structs = self._net_pair(net_white, net_black)
        if out is None:
            mk = lambda on, dt: t.empty((N, trials), dtype=dt, device=self.device) if on else None  # noqa: E731
            out = PlayoutResult(t.empty((N, 4), dtype=t.int32, device=self.device), trials, mk(per_trial, t.int8),
                                mk(per_trial, t.int32), mk(leaf, t.float32))
        elif tuple(out.sums.shape) != (N, 4) or out.trials != trials or out.sums.device != self.device:
            raise ValueError("out must be a PlayoutResult of the same roots and trials on this device")
        tail = ()
        if self._kind.turn_scratch:
            scratch = self._turn_scratch(scratch, N * trials)
            tail = (_lib.ptr(scratch), int(scratch.numel()))
        self.handle.call(self._kind.playout, N, _lib.ptr(roots), trials, max_plies,
                         *(ctypes.byref(m) if m is not None else None for m in structs), int(seed) & (2 ** 64 - 1),
                         int(id_base), _lib.PLAYOUT_COMMON_DICE if common_dice else 0, _lib.ptr(out.sums),
                         _lib.ptr(out.outcome), _lib.ptr(out.length), _lib.ptr(out.leaf), *tail, self._s())
        self._keep = (roots, net_white, net_black, structs, out, scratch)
        return out

    def playout_targets(self, result, roots=None, leaf=False, out=None):
        """A playout call's sums as regression targets for td.ValueFitter
        (narde_playout_targets), by pick_playout()'s
        score arithmetic: per root the mean outcome of its finished trials
        and weight 1 -- target 0 and weight 0 where none finished --, or with
        leaf=True the truncated mean (points + the unfinished trials' leaves)
        / trials and weight 1.  result: playout()'s PlayoutResult or a (sums,
        trials[, leaf]) tuple.  roots: the (N, 8) records the playouts started
        from; given, a root in which a side already has its 15 checkers off
        (a terminal row's record, the none record) gets target 0, weight 0.
        Returns (target, weight), (N,) float32; out: an earlier pair to write
        into.  No synchronise."""
        t = self.torch
        sums, trials, lf = self._playout_sums(result, leaf)
        if (sums.dim() != 2 or sums.shape[1] != 4 or sums.shape[0] < 1 or sums.dtype != t.int32
                or not sums.is_contiguous() or sums.device != self.device):
            raise ValueError("result must hold (N, 4) int32 sums on this device")
        N = int(sums.shape[0])
        if lf is not None and (tuple(lf.shape) != (N, trials) or lf.dtype != t.float32 or not lf.is_contiguous()):
            raise ValueError("leaf must be (N, trials) float32")
        if roots is not None:
            self._check_records(roots, "roots must be the playouts' contiguous (N, 8) int32 records", N, N)
        if out is not None:
            target, weight = out
        else:
            target = t.empty(N, dtype=t.float32, device=self.device)
            weight = t.empty(N, dtype=t.float32, device=self.device)
        _lib.check(self.handle.lib.narde_playout_targets(self.device.index, N, trials, _lib.ptr(sums), _lib.ptr(lf),
                                                         _lib.ptr(roots), _lib.ptr(target), _lib.ptr(weight), self._s()),
                   "narde_playout_targets")
        self._keep = (sums, lf, roots)
        return target, weight

    def rollout_launcher(self, plies, bufs, events=None, totals=None):
        """rollout(plies, bufs) pre-bound: a zero-argument callable that makes
        exactly one ctypes call (one kernel launch on the stream current
        NOW), for hot loops where the per-call Python of rollout() would
        show (the buffers must stay alive and unmoved while it is used).
        With events, the launch is pre-bound in the library
        (narde_rollout_plan_*: one pointer per call; $NARDE_ROLLOUT_PLAN=0
        takes narde_rollout_timed's per-call arguments instead).
        events = (start, stop) torch.cuda.Event or TimingEvent (either None): recorded on
        that stream right before / after the launch, inside the same call
        (narde_rollout_timed); a torch event must have been recorded once
        already (it creates its HIP event at its first record).
        totals: a (wg_rows(B), 3) int64 device tensor the launch fills with
        the statistics after it summed per 256 envs (.sum(0) = the
        handle's {episodes, white points, black points}) -- no second launch."""
        for v in bufs.values():
            if v is not None and v.shape[0] < plies:
                raise ValueError("rollout buffer shorter than plies")
        if totals is not None:
            t = self.torch
            if (tuple(totals.shape) != (_lib.wg_rows(self.num_envs), 3) or totals.dtype != t.int64
                    or totals.device != self.device or not totals.is_contiguous()):
                raise ValueError(f"totals must be a contiguous ({_lib.wg_rows(self.num_envs)}, 3) int64 "
                                 "tensor on the env's device")
            if plies <= 0:
                raise ValueError("totals need a launch (plies > 0)")
            events = events if events is not None else (None, None)
        bufargs = (_lib.ptr(bufs["obs"]), _lib.ptr(bufs["reward"]), _lib.ptr(bufs["terminated"]),
                   _lib.ptr(bufs["truncated"]), _lib.ptr(bufs["legal"]), _lib.ptr(bufs["actions"]))
        if events is None:
            name = self._kind.rollout
            fn = getattr(self.handle.lib, name)
            args = (self.handle.h, int(plies)) + bufargs + (self._s(),)
        else:
            evs = []
            for ev in events:
                if isinstance(ev, TimingEvent):
                    evs.append(ctypes.c_void_p(ev.handle))
                    continue
                if ev is not None and not ev.cuda_event:
                    raise ValueError("record each event once before binding it (its HIP event is created then)")
                evs.append(ctypes.c_void_p(ev.cuda_event) if ev is not None else None)
            fn, name = self.handle.lib.narde_rollout_timed, "narde_rollout_timed"
            args = (self.handle.h, int(self.full), int(plies)) + bufargs + (evs[0], evs[1], _lib.ptr(totals),
                                                                            self._s())
            if int(plies) > 0 and os.environ.get("NARDE_ROLLOUT_PLAN", "1") == "1":
                # round 6: the same launch pre-bound in the library
                # (narde_rollout_plan_*): the timed call is one pointer
                plan = ctypes.c_void_p()
                _lib.check(self.handle.lib.narde_rollout_plan_create(*args, ctypes.byref(plan)),
                           "narde_rollout_plan_create")
                fn, name, args = self.handle.lib.narde_rollout_plan_launch, "narde_rollout_plan_launch", (plan,)

        def launch():
            rc = fn(*args)
            if rc:
                _lib.check(rc, name)

        if fn is self.handle.lib.narde_rollout_plan_launch:
            weakref.finalize(launch, self.handle.lib.narde_rollout_plan_destroy, args[0])

        launch.bufs = bufs  # keeps the buffers referenced as long as the launcher
        launch.events = events
        launch.totals = totals
        return launch

    def stats(self, out=None):
        """(B,3) int32 {episodes finished, white points, black points} (into
        `out` if given: a preallocated (B,3) int32 device tensor)."""
        if out is None:
            out = self.torch.empty((self.num_envs, 3), dtype=self.torch.int32, device=self.device)
        elif (tuple(out.shape) != (self.num_envs, 3) or out.dtype != self.torch.int32
              or out.device != self.device or not out.is_contiguous()):
            raise ValueError("out must be a contiguous (B,3) int32 tensor on the env's device")
        self.handle.call("narde_get_stats", _lib.ptr(out), self._s())
        return out

    def totals(self, out=None):
        """(64,3) int64 partial sums of stats() over contiguous env ranges
        (narde_get_totals: one launch); .sum(0) gives {episodes, white
        points, black points} of the handle (into `out` if given)."""
        if out is None:
            out = self.torch.empty((_lib.TOTAL_ROWS, 3), dtype=self.torch.int64, device=self.device)
        elif (tuple(out.shape) != (_lib.TOTAL_ROWS, 3) or out.dtype != self.torch.int64
              or out.device != self.device or not out.is_contiguous()):
            raise ValueError("out must be a contiguous (64,3) int64 tensor on the env's device")
        self.handle.call("narde_get_totals", _lib.ptr(out), self._s())
        return out

    def totals_launcher(self, out):
        """totals(out) pre-bound: a zero-argument callable making exactly one
        ctypes call (one launch on the stream current NOW); returns out."""
        t = self.torch
        if (tuple(out.shape) != (_lib.TOTAL_ROWS, 3) or out.dtype != t.int64 or out.device != self.device
                or not out.is_contiguous()):
            raise ValueError("out must be a contiguous (64,3) int64 tensor on the env's device")
        fn, args = self.handle.lib.narde_get_totals, (self.handle.h, _lib.ptr(out), self._s())

        def launch():
            rc = fn(*args)
            if rc:
                _lib.check(rc, "narde_get_totals")
            return out

        launch.out = out
        return launch

    def get_state(self):
        B, t, dev = self.num_envs, self.torch, self.device
        st = dict(board=t.empty((B, 24), dtype=t.int8, device=dev),
                  off=t.empty((B, 2), dtype=t.uint8, device=dev),
                  first_turn=t.empty((B, 2), dtype=t.uint8, device=dev),
                  player=t.empty(B, dtype=t.int8, device=dev),
                  elapsed=t.empty(B, dtype=t.int16, device=dev))
        self.handle.call("narde_get_state", _lib.ptr(st["board"]), _lib.ptr(st["off"]),
                         _lib.ptr(st["first_turn"]), _lib.ptr(st["player"]), _lib.ptr(st["elapsed"]),
                         self._s())
        return st

    def set_state(self, board, off, first_turn, player, elapsed=None):
        B, t = self.num_envs, self.torch
        b = self._dev(board, t.int8, (B, 24))
        o = self._dev(off, t.uint8, (B, 2))
        f = self._dev(first_turn, t.uint8, (B, 2))
        p = self._dev(player, t.int8, (B,))
        e = None if elapsed is None else self._dev(elapsed, t.int16, (B,))
        self.handle.call("narde_set_state", _lib.ptr(b), _lib.ptr(o), _lib.ptr(f), _lib.ptr(p),
                         _lib.ptr(e), self._s())
        self._keep = (b, o, f, p, e)  # keep inputs alive until the kernel has read them

    def apply_moves(self, moves, player=None):
        """execute_rotated_move per env; moves (B,2) int8 (to=24 for off, from<0 skips)."""
        B, t = self.num_envs, self.torch
        m = self._dev(moves, t.int8, (B, 2))
        p = None if player is None else self._dev(player, t.int8, (B,))
        self.handle.call("narde_apply_moves", _lib.ptr(m), _lib.ptr(p), self._s())
        self._keep = (m, p)

    def close(self):
        self.handle.close()


class TimingEvent:
    """A HIP event made by the library (narde_timing_event_create) for
    rollout_launcher(..., events=...).  flags: DISABLE_SYSTEM_FENCE (default)
    makes the record a timing-only marker -- no system-scope cache write-back
    and invalidate when it completes, so the marker after a launch does not
    lengthen the span it measures; 0 = HIP's default event (what a
    torch.cuda.Event is)."""

    DISABLE_SYSTEM_FENCE = 0x20000000

    def __init__(self, device=None, flags=DISABLE_SYSTEM_FENCE):
        import torch

        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.narde_timing_event_create(dev.index or 0, int(flags), ctypes.byref(h)),
                   "narde_timing_event_create")
        self.handle = h.value

    def elapsed_ms(self, stop):
        """Milliseconds from this event to `stop` (both recorded and complete)."""
        ms = ctypes.c_float()
        _lib.check(self._lib.narde_timing_event_elapsed_ms(ctypes.c_void_p(self.handle),
                                                            ctypes.c_void_p(stop.handle), ctypes.byref(ms)),
                   "narde_timing_event_elapsed_ms")
        return float(ms.value)

    def close(self):
        if self.handle:
            self._lib.narde_timing_event_destroy(ctypes.c_void_p(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
