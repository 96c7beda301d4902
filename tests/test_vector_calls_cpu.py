"""VecNardeEnv's Python, its learners and players on a fake handle: which
entry points a method calls, in which order and with which arguments, what it
raises, and what it keeps alive.  No device: a test-local subclass replaces
__init__ and _s(), and the handle records every call -- a NULL as NULL, a
pointer as the tensor it belongs to (matched back by data_ptr() to what the
test passed, the method returned or the env keeps), a scalar by value.  The
expected traces are tests/golden/vector_calls.json, recorded from the modules
as they stood before their rule-set twins were folded (`PYTHONPATH=gym-narde_amd
python tests/test_vector_calls_cpu.py --record` writes it: only when a call is
meant to change); the error texts are literals here.
"""
import ctypes
import json
import math
import os
import sys
import types

import pytest
import torch

from gym_narde import _lib, td, value_play, vector
from gym_narde.value_net import HIDDEN_ACTS, OUT_ACTS
from gym_narde.vector import PlayoutResult, VecNardeEnv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vector_calls.json")
B = 3
TOTAL = 5  # what the fake's sizing call reports in offsets[B]
WAVES = 7  # what the fake's occupancy query reports
STREAM = 0x5EED
RULES = ("ref2", "full4")
# a method and its rule-set twin
M = {"ref2": dict(expand="afterstates", scored="scored_afterstates", look="lookahead_afterstates",
                  rec="recorded_afterstates", pick="pick_afterstate", roll="value_rollout",
                  league="value_rollout_league", bufs="value_rollout_buffers", field="codes", shape=(2,),
                  dtype=torch.int16, tuple=vector.Afterstates),
     "full4": dict(expand="turn_afterstates", scored="scored_turn_afterstates", look="lookahead_turn_afterstates",
                   rec="recorded_turn_afterstates", pick="pick_turn", roll="turn_value_rollout",
                   league="turn_value_rollout_league", bufs="turn_value_rollout_buffers", field="play", shape=(4, 2),
                   dtype=torch.int8, tuple=vector.TurnAfterstates)}


class FakeLib:
    """The library's direct calls (narde_net_table, narde_step, ...)."""

    def __init__(self, handle):
        self._handle = handle

    def __getattr__(self, name):
        if not name.startswith("narde_"):
            raise AttributeError(name)
        return lambda *args: self._handle.record(name, args)


class FakeHandle:
    def __init__(self):
        self.h = ctypes.c_void_p(0xABCD)
        self.calls = []
        self.lib = FakeLib(self)
        self.ply = 11

    def call(self, name, *args):
        self.record(name, args)

    def record(self, name, args):
        self.calls.append((name, args))
        if name in ("narde_afterstates", "narde_turn_afterstates") and args[1] == 0:
            # the sizing call: the total through the offsets pointer
            ctypes.cast(args[2], ctypes.POINTER(ctypes.c_int32))[B] = TOTAL
        if name == "narde_turn_value_rollout_waves":
            args[0]._obj.value = WAVES
        return 0


class Env(VecNardeEnv):
    def __init__(self, rules="ref2", autoreset=True):
        self.rules, self.full = rules, rules == "full4"
        self.torch, self.device = torch, torch.device("cpu")
        self.num_envs, self.autoreset = B, autoreset
        self.handle = FakeHandle()
        self.obs = torch.zeros((B, 24), dtype=torch.int32)
        self.reward = torch.zeros(B, dtype=torch.int32)
        self.terminated = torch.zeros(B, dtype=torch.uint8)
        self.truncated = torch.zeros(B, dtype=torch.uint8)
        self.legal = torch.zeros(B, dtype=torch.int64)
        self.actions_used = torch.zeros((B, 2), dtype=torch.int16)
        self.played = torch.zeros(B, dtype=torch.int64)
        self._look_scratch = None
        self._keep = None
        if hasattr(self, "_bind"):  # the rule set's descriptor and step()'s plumbing, as __init__ resolves them
            self._bind()
        else:
            lib = self.handle.lib
            self._step_fn = lib.narde_step_full if self.full else lib.narde_step
            self._step_out = tuple(_lib.ptr(t) for t in (
                (self.obs, self.reward, self.terminated, self.truncated, self.legal, self.played) if self.full else
                (self.obs, self.reward, self.terminated, self.truncated, self.legal, self.actions_used)))

    def _s(self):
        return ctypes.c_void_p(STREAM)


class Net:
    """What the calls read of a value_net.ValueMLP, on the host."""

    def __init__(self, name, hidden=4, device="cpu"):
        self.name, self.hidden, self.hidden_act, self.out_act = name, hidden, "sigmoid", "tanh"
        self.l1 = types.SimpleNamespace(weight=torch.zeros((hidden, 198), device=device), bias=torch.zeros(hidden))
        self.l2 = types.SimpleNamespace(weight=torch.zeros((1, hidden)), bias=torch.zeros(1))
        self._w1t = torch.zeros((198, hidden))

    def pack(self):
        return self

    def struct(self):
        return _lib.ValueMlp(self._w1t.data_ptr(), self.hidden, self.l1.bias.data_ptr(), self.l2.weight.data_ptr(),
                             self.l2.bias.data_ptr(), self.hidden, HIDDEN_ACTS[self.hidden_act],
                             OUT_ACTS[self.out_act])

    def __call__(self, feat):
        return feat.sum(1)


class Unpacked(Net):
    """A net whose struct() raises (a ValueMLP off the GPU does), on another device."""

    def __init__(self):
        super().__init__("unpacked", device="meta")

    def struct(self):
        raise ValueError("no struct")


def _leaves(label, obj, out):
    """(label, leaf) of every tensor, net and struct inside obj."""
    if isinstance(obj, (torch.Tensor, Net, ctypes.Structure)) or obj is None:
        out.append((label, obj))
    elif isinstance(obj, PlayoutResult):
        for f in ("sums", "outcome", "length", "leaf"):
            _leaves(f"{label}.{f}", getattr(obj, f), out)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _leaves(f"{label}[{k}]", v, out)
    elif hasattr(obj, "_fields"):
        for k in obj._fields:
            _leaves(f"{label}.{k}", getattr(obj, k), out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _leaves(f"{label}[{i}]", v, out)
    else:
        out.append((label, obj))
    return out


class Ctx:
    """One scenario: the env, two nets, and the names of what the test passes."""

    def __init__(self, rules, **kw):
        self.rules, self.m = rules, M[rules]
        self.env = Env(rules, **kw)
        self.net, self.other = Net("net"), Net("other")
        self.named = []
        self.temporaries = False  # the scenario's callee passes tensors of its own that it does not keep

    def a(self, label, obj):
        self.named.append((label, obj))
        return obj

    def z(self, label, shape, dtype):
        return self.a(label, torch.zeros(shape, dtype=dtype))

    def call(self, key, *args, **kw):
        return getattr(self.env, self.m[key])(*args, **kw)

    def aft(self, cap, rows=None, feat=False, obs=False, label="aft"):
        m, rows = self.m, cap if rows is None else rows
        mk = lambda shape, dt: torch.zeros((rows,) + shape, dtype=dt)  # noqa: E731
        return self.a(label, m["tuple"](torch.zeros(B + 1, dtype=torch.int32), mk((), torch.int32),
                                        mk(m["shape"], m["dtype"]), mk((198,), torch.float32) if feat else None,
                                        mk((24,), torch.int32) if obs else None, mk((), torch.int8), cap))

    def bufs(self, plies, **kw):
        return self.a("bufs", self.call("bufs", plies, **kw))

    def scratch(self, waves=2):
        return self.z("scratch", _lib.turn_rollout_scratch_bytes(waves), torch.uint8) if self.env.full else None

    def table(self, n=2):
        return self.z("table", _lib.league_table_bytes(n), torch.uint8)

    def forget(self):
        del self.env.handle.calls[:]


def _ten(x):
    return f"{tuple(x.shape)}:{str(x.dtype)[6:]}"


def describe(c, ret):
    """The scenario's trace: its calls, what it returned, what the env keeps."""
    env = c.env
    pool = []
    for label, obj in c.named:
        _leaves(label, obj, pool)
    _leaves("ret", ret, pool)
    for name in ("_look_scratch", "_records_look_scratch", "_turn_rollout_scratch", "_playout_scratch"):
        _leaves(f"env.{name}", getattr(env, name, None), pool)
    for name in ("obs", "reward", "terminated", "truncated", "legal", "actions_used", "played"):
        _leaves(f"env.{name}", getattr(env, name), pool)
    _leaves("keep", getattr(env, "_keep", None), pool)
    for net in (c.net, c.other):
        pool.append((f"{net.name}._w1t", net._w1t))
    by_ptr, by_id = {}, {}
    for label, x in pool:
        if isinstance(x, torch.Tensor) and x.numel():
            by_ptr.setdefault(x.data_ptr(), f"{label}{_ten(x)}")
        if x is not None and not isinstance(x, (int, float, str, bool)):
            by_id.setdefault(id(x), label)

    def mlp(s):
        return by_ptr.get(s.w1t, "?").split(".")[0]

    def arg(a):
        if a is None:
            return "NULL"
        if isinstance(a, ctypes.c_void_p):
            if a.value is None:
                return "NULL"
            label = {STREAM: "stream", 0xABCD: "h"}.get(a.value) or by_ptr.get(a.value, "ptr")
            # (a tensor the callee made and dropped may share its address with a later one)
            return "ptr" if c.temporaries and label.startswith("keep") else label
        if isinstance(a, ctypes.Array):
            return "mlps[" + ",".join(mlp(s) for s in a) + "]"
        if hasattr(a, "_obj"):  # ctypes.byref()
            o = a._obj
            return f"&{type(o).__name__}({mlp(o)})" if isinstance(o, ctypes.Structure) else f"&{type(o).__name__}"
        if isinstance(a, float) and math.isnan(a):
            return "nan"
        return repr(a)

    def leaf(x):
        if x is None:
            return "None"
        if isinstance(x, torch.Tensor):
            return by_id.get(id(x)) or by_ptr.get(x.data_ptr() if x.numel() else -1, _ten(x))
        if isinstance(x, Net):
            return f"net:{x.name}"
        if isinstance(x, ctypes.Structure):
            return f"{type(x).__name__}({mlp(x)})"
        return repr(x)

    def shown(label, x):
        if not isinstance(x, torch.Tensor):
            return f"{label}={leaf(x)}"
        first = by_ptr.get(x.data_ptr()) if x.numel() else None
        same = f" is {first}" if first and not first.startswith("ret") and not first.startswith("keep") else ""
        return f"{label}{_ten(x)}{same}"

    keep = sorted({leaf(x) for label, x in _leaves("keep", getattr(env, "_keep", None), []) if not label == "keep"})
    # (the struct objects, not copies of them: the C side holds pointers into what byref() was given)
    return {"calls": [f"{name}({', '.join(arg(a) for a in args)})" for name, args in env.handle.calls],
            "ret": [shown(label, x) for label, x in _leaves("ret", ret, [])],
            "keep": keep}


def rec(n=4):
    return torch.zeros((n, 8), dtype=torch.int32)


# ---------------------------------------------------------------- scenarios
# name -> f(c); run for both rule sets.  A scenario returns what to show as ret.
S = {}


def scenario(f):
    S[f.__name__] = f
    return f


@scenario
def expand_neither(c):
    return c.call("expand", c.z("dice", (B, 2), torch.uint8))


@scenario
def expand_cap5_obs(c):
    return c.call("expand", cap=5, feat=False, obs=True)


@scenario
def expand_cap1(c):
    return c.call("expand", c.z("dice", (B, 2), torch.uint8), cap=1)


@scenario
def expand_cap0(c):
    return c.call("expand", cap=0)


@scenario
def expand_out(c):
    return c.call("expand", out=c.aft(5, feat=True, obs=True, label="out"))


@scenario
def expand_out_cap1(c):
    return c.call("expand", cap=1, out=c.aft(5, label="out"))


@scenario
def expand_out_cap0(c):
    return c.call("expand", cap=0, out=c.aft(5, feat=True, label="out"))


@scenario
def scored_neither(c):
    return c.call("scored", c.a("net", c.net))


@scenario
def scored_cap5_mover(c):
    return c.call("scored", c.net, c.z("dice", (B, 2), torch.uint8), cap=5, perspective="mover")


@scenario
def scored_cap1(c):
    return c.call("scored", c.net, cap=1)


@scenario
def scored_cap0(c):
    return c.call("scored", c.net, cap=0)


@scenario
def scored_out_pair(c):
    return c.call("scored", c.net, out=(c.aft(5, feat=True, label="out"), c.z("values", 6, torch.float32)))


@scenario
def scored_out_alone_cap1(c):
    return c.call("scored", c.net, cap=1, out=c.aft(5, label="out"))


@scenario
def scored_out_cap0(c):
    return c.call("scored", c.net, cap=0, out=(c.aft(5, label="out"), c.z("values", 5, torch.float32)))


@scenario
def look_neither(c):
    return c.call("look", c.net)


@scenario
def look_cap5_then_cap1(c):  # the scratch is not made again for a smaller cap
    c.a("first", c.call("look", c.net, cap=5))
    first = c.a("first_scratch", c.env._look_scratch)
    ret = c.call("look", c.net, c.z("dice", (B, 2), torch.uint8), cap=1)
    assert c.env._look_scratch is first
    return ret


@scenario
def look_cap1_then_cap5(c):  # and grows with it
    c.a("first", c.call("look", c.net, cap=1))
    first = c.a("first_scratch", c.env._look_scratch)
    ret = c.call("look", c.net, cap=5)
    assert c.env._look_scratch is not first
    return ret


@scenario
def look_cap0(c):
    ret = c.call("look", c.net, cap=0)
    assert c.env._look_scratch is None
    return ret


@scenario
def look_out(c):
    return c.call("look", c.net, out=(c.aft(5, label="out"), c.z("values", 5, torch.float32)))


@scenario
def recorded_neither(c):
    return c.call("rec", c.net)


@scenario
def recorded_no_net_neither(c):
    return c.call("rec", None, c.z("dice", (B, 2), torch.uint8))


@scenario
def recorded_cap5(c):
    return c.call("rec", c.net, cap=5)


@scenario
def recorded_cap1_no_net(c):
    return c.call("rec", None, cap=1)


@scenario
def recorded_cap0(c):
    return c.call("rec", c.net, cap=0)


@scenario
def recorded_out(c):
    return c.call("rec", c.net, out=(c.aft(5, feat=True, label="out"), c.z("values", 5, torch.float32),
                                     c.a("records", rec(6))))


@scenario
def recorded_out_no_net_cap1(c):
    return c.call("rec", None, cap=1, out=(c.aft(5, label="out"), None, c.a("records", rec(5))))


@scenario
def recorded_out_cap0(c):
    return c.call("rec", c.net, cap=0, out=(c.aft(5, label="out"), c.z("values", 5, torch.float32),
                                            c.a("records", rec(5))))


@scenario
def top_rows_records(c):
    return c.env.top_rows(c.aft(5), c.z("values", (7, 1), torch.float32), 2, c.a("records", rec(5)), "mover")


@scenario
def top_rows_plain_cap1(c):
    return c.env.top_rows(c.aft(1), c.z("values", 1, torch.float32), 1)


@scenario
def top_rows_strided_out(c):
    v = c.z("values2", (5, 2), torch.float32)[:, 0]
    out = (c.z("sel", (B, 2), torch.int32), c.z("roots", (B * 2, 8), torch.int32))
    return c.env.top_rows(c.aft(5), v, 2, c.a("records", rec(5)), out=out)


@scenario
def top_rows_cap0(c):
    sel, roots = c.env.top_rows(c.aft(0, rows=1), c.z("values", 0, torch.float32), 2, c.a("records", rec(1)))
    assert (sel == -1).all() and (roots[:, 6] == _lib.RECORD_NONE_WORD6).all() and roots.sum() == 6 * 0xFF
    return sel, roots


@scenario
def top_rows_cap0_no_records(c):
    sel, roots = c.env.top_rows(c.aft(0, rows=1), c.z("values", 0, torch.float32), 3)
    assert (sel == -1).all() and roots is None
    return sel, roots


@scenario
def pick_greedy(c):
    return c.call("pick", c.aft(5), c.z("values", 5, torch.float32))


@scenario
def pick_cap1_mover(c):
    return c.call("pick", c.aft(1), c.z("values", (1, 1), torch.float32), "mover")


@scenario
def pick_explore_numbers(c):
    return c.call("pick", c.aft(5), c.z("values", 5, torch.float32), "white", 0.25, 9, seed=-1)


@scenario
def pick_explore_tensors(c):
    return c.call("pick", c.aft(5), c.z("values", 5, torch.float32), epsilon=c.z("eps", (), torch.float32),
                  tag=c.z("tag", (), torch.int64), seed=3)


@scenario
def pick_cap0(c):
    actions, row = c.call("pick", c.aft(0, rows=1), c.z("values", 0, torch.float32), epsilon=0.5, tag=1)
    assert (actions == (-1 if c.env.full else 0)).all() and (row == -1).all()
    assert tuple(actions.shape) == (B,) + c.m["shape"] and actions.dtype == c.m["dtype"]
    return actions, row


def _result(c, k=2, trials=3, leaf=True):
    return c.a("result", PlayoutResult(torch.zeros((B * k, 4), dtype=torch.int32), trials, None, None,
                                       torch.zeros((B * k, trials)) if leaf else None))


@scenario
def pick_playout_result(c):
    return c.env.pick_playout(c.aft(5), c.z("values", 5, torch.float32), c.z("sel", (B, 2), torch.int32), _result(c))


@scenario
def pick_playout_leaf(c):
    return c.env.pick_playout(c.aft(5), c.z("values", 5, torch.float32), c.z("sel", (B, 2), torch.int32), _result(c),
                              leaf=True)


@scenario
def pick_playout_tuple_out(c):
    out = (c.z("actions", (B,) + c.m["shape"], c.m["dtype"]), c.z("row", B, torch.int32),
           c.z("score", (B, 1), torch.float32))
    res = (c.z("sums", (B, 4), torch.int32), 3.0)
    return c.env.pick_playout(c.aft(1), c.z("values", 1, torch.float32), c.z("sel", (B, 1), torch.int32), res, out=out)


@scenario
def pick_playout_tuple_leaf(c):
    res = (c.z("sums", (B, 4), torch.int32), 3, c.z("leaf", (B, 3), torch.float32))
    return c.env.pick_playout(c.aft(1), c.z("values", 1, torch.float32), c.z("sel", (B, 1), torch.int32), res, True)


@scenario
def pick_playout_cap0(c):
    actions, row, score = c.env.pick_playout(c.aft(0, rows=1), c.z("values", 0, torch.float32),
                                             c.z("sel", (B, 2), torch.int32), _result(c, leaf=False))
    assert (actions == (-1 if c.env.full else 0)).all() and (row == -1).all() and torch.isnan(score).all()
    assert tuple(actions.shape) == (B,) + c.m["shape"] and actions.dtype == c.m["dtype"]
    return actions, row, score


@scenario
def pick_slots_plain(c):
    return c.env.pick_slots(c.aft(5), c.z("values", 5, torch.float32), c.z("sel", (B, 2), torch.int32),
                            c.z("slot_score", (B * 2,), torch.float32))


@scenario
def pick_slots_out_cap1(c):
    out = (c.z("actions", (B,) + c.m["shape"], c.m["dtype"]), c.z("row", B, torch.int32),
           c.z("score", (B, 2), torch.float32))
    return c.env.pick_slots(c.aft(1), c.z("values", (1, 1), torch.float32), c.z("sel", (B, 2), torch.int32),
                            c.z("slot_score", (B, 2), torch.float32), out=out)


@scenario
def pick_slots_cap0(c):
    actions, row, score = c.env.pick_slots(c.aft(0, rows=1), c.z("values", 0, torch.float32),
                                           c.z("sel", (B, 2), torch.int32), c.z("slot_score", (B, 2), torch.float32))
    assert (actions == (-1 if c.env.full else 0)).all() and (row == -1).all() and torch.isnan(score).all()
    assert tuple(actions.shape) == (B,) + c.m["shape"] and actions.dtype == c.m["dtype"]
    return actions, row, score


@scenario
def lookahead_records_plain(c):
    return c.env.lookahead_records(c.a("records", rec(4)), c.net)


@scenario
def lookahead_records_out_grow(c):  # full4: the scratch kept for a smaller n, made again for a larger one
    c.a("first", c.env.lookahead_records(c.a("records1", rec(4)), c.net))
    first = c.a("first_scratch", getattr(c.env, "_records_look_scratch", None))
    c.a("second", c.env.lookahead_records(c.a("records2", rec(2)), c.net))
    assert getattr(c.env, "_records_look_scratch", None) is first and (first is None) == (not c.env.full)
    c.forget()
    ret = c.env.lookahead_records(c.a("records", rec(6)), c.net, out=c.z("out", 6, torch.float32))
    assert c.env.full == (getattr(c.env, "_records_look_scratch", None) is not first)
    return ret


@scenario
def rollout_defaults(c):
    return c.call("roll", 2, c.net)


@scenario
def rollout_twice(c):  # full4: the scratch made by the first call serves the second
    c.a("first", c.call("roll", 1, c.net))
    first = getattr(c.env, "_turn_rollout_scratch", None)
    assert (first is not None) == c.env.full
    ret = c.call("roll", 1, c.other, c.net, seed=2 ** 64 + 5)
    assert getattr(c.env, "_turn_rollout_scratch", None) is first
    return ret


@scenario
def rollout_black_random_explore(c):
    return c.call("roll", 2, c.net, None, 0.125, 4, 7, c.bufs(3, records=True))


@scenario
def rollout_white_random_tensors(c):
    kw = dict(scratch=c.scratch()) if c.env.full else {}
    return c.call("roll", 1, None, c.other, epsilon=c.z("eps", (), torch.float32), tag=c.z("tag", (), torch.int64),
                  bufs=c.bufs(1, dice=False, value=False, terminated=False), **kw)


@scenario
def rollout_buffers(c):
    return [c.call("bufs", 2), c.call("bufs", 3.0, records=True),
            c.call("bufs", 1, False, False, False, False, False, False), c.call("bufs", 1, value=False, records=True)]


@scenario
def waves_and_scratch(c):
    e = c.env
    return [e.turn_value_rollout_waves(), e.turn_value_rollout_scratch(), e.turn_value_rollout_scratch(2)]


@scenario
def net_table_plain(c):
    t = c.env.net_table([c.net, c.other, c.net])
    assert c.env._league_nets[t.data_ptr()] == (c.net, c.other, c.net)
    return t


@scenario
def net_table_out(c):
    out = c.z("out", 200, torch.uint8)
    t = c.env.net_table(iter([c.net]), out=out)
    assert c.env._league_nets[t.data_ptr()] == (c.net,) and t.data_ptr() == out.data_ptr()
    return t


@scenario
def league_defaults(c):
    return c.call("league", 2, c.table(), c.z("white", B, torch.int32), c.z("black", B, torch.int32))


@scenario
def league_explore_bufs(c):
    kw = dict(scratch=c.scratch()) if c.env.full else {}
    return c.call("league", 1, c.table(3), c.z("white", B, torch.int32), c.z("black", B, torch.int32), 0.5, 2, -3,
                  c.bufs(2, records=True), **kw)


@scenario
def league_twice(c):
    w, b = c.z("white", B, torch.int32), c.z("black", B, torch.int32)
    c.a("first", c.call("league", 1, c.table(), w, b))
    first = getattr(c.env, "_turn_rollout_scratch", None)
    ret = c.call("league", 1, c.table(1), w, b, epsilon=c.z("eps", (), torch.float32),
                 tag=c.z("tag", (), torch.int64))
    assert getattr(c.env, "_turn_rollout_scratch", None) is first and (first is not None) == c.env.full
    return ret


@scenario
def playout_defaults(c):
    return c.env.playout(c.a("roots", rec(2)), 3, c.net)


@scenario
def playout_dict_per_trial_leaf(c):
    roots = dict(board=torch.zeros((2, 24), dtype=torch.int8), off=torch.zeros((2, 2), dtype=torch.uint8),
                 first_turn=torch.zeros((2, 2), dtype=torch.uint8), player=torch.ones(2, dtype=torch.int8))
    return c.env.playout(c.a("roots", roots), 2, c.net, None, max_plies=9, seed=-2, id_base=4, common_dice=True,
                         per_trial=True, leaf=True)


@scenario
def playout_out_scratch(c):
    out = c.a("out", PlayoutResult(torch.zeros((2, 4), dtype=torch.int32), 3, None, torch.zeros((2, 3), dtype=torch.int32)))
    return c.env.playout(c.a("roots", rec(2)), 3, None, c.other, scratch=c.scratch(), out=out)


@scenario
def playout_grow(c):  # full4: one occupancy query; the scratch kept for fewer trials, made again for more
    e = c.env
    c.a("first", e.playout(c.a("roots1", rec(1)), 2, c.net))
    first = c.a("first_scratch", getattr(e, "_playout_scratch", None))
    assert (first is not None) == e.full and getattr(e, "_playout_waves", None) == (WAVES if e.full else None)
    c.a("second", e.playout(c.a("roots2", rec(1)), 1, c.net))
    assert getattr(e, "_playout_scratch", None) is first
    ret = e.playout(c.a("roots", rec(2)), 5, c.net)
    assert e.full == (getattr(e, "_playout_scratch", None) is not first)
    return ret


@scenario
def playout_targets_result(c):
    return c.env.playout_targets(_result(c, 1, 3), leaf=True)


@scenario
def playout_targets_tuple_out(c):
    out = (c.z("target", B, torch.float32), c.z("weight", B, torch.float32))
    return c.env.playout_targets((c.z("sums", (B, 4), torch.int32), 4.0), c.a("roots", rec(B)), out=out)


@scenario
def playout_targets_no_leaf(c):
    return c.env.playout_targets((c.z("sums", (B, 4), torch.int32), 2, c.z("leaf", (B, 2), torch.float32)))


@scenario
def step_selfplay_rollout(c):
    e = c.env
    actions = c.z("actions", (B,) + c.m["shape"], c.m["dtype"])
    out = [e.step(), e.step(actions, c.z("dice", (B, 2), torch.uint8))]
    e.selfplay(4.0)
    out.append(e.rollout(2))
    launch = e.rollout_launcher(2, c.a("bufs", e.rollout_buffers(2, obs=False)))
    launch()
    return out


def _learner(c, kind):
    if kind == "window":
        return td.WindowTDLambdaLearner(c.env, c.net, 0.1, 0.7, 2, epsilon=0.25, seed=5)
    if kind == "window_greedy":
        return td.WindowTDLambdaLearner(c.env, c.net, 0.1, 0.7, 3)
    if kind == "playout":
        return td.PlayoutTargetLearner(c.env, c.net, 0.1, 2, 3, epsilon=0.25, seed=5)
    return td.LookaheadTargetLearner(c.env, c.net, 0.1, 2, every=2, epsilon=0.5)


def _play_twice(c, kind):
    L = _learner(c, kind)
    c.a("L.bufs", L.bufs), c.a("L._roll_scratch", L._roll_scratch), c.a("L._eps", L._eps), c.a("L._tag", L._tag)
    assert (L._roll_scratch is not None) == c.env.full and "records" in L.bufs
    assert list(L.bufs) == ["dice", "play" if c.env.full else "actions", "value", "reward", "terminated", "truncated",
                            "records"]
    greedy = kind == "window_greedy"
    assert (L._eps is None) == greedy and (L._tag is None) == greedy
    own = sum(x.numel() * x.element_size() for x in list(L.bufs.values()) + [L._roll_scratch] if x is not None)
    rest = {"window": 4 * (2 * B + _lib.td_window_scratch_floats(B, 2, 4)),
            "window_greedy": 4 * (3 * B + _lib.td_window_scratch_floats(B, 3, 4))}.get(kind)
    if rest is None:
        N = B * (1 if kind == "lookahead" else 2)
        rest = N * 40 + L.fitter.memory_bytes()
    assert L.memory_bytes() == own + rest
    assert L.play() is L.bufs and L.play() is L.bufs
    assert greedy or int(L._tag) == 2 * L.plies
    assert kind.startswith("window") or L.windows == 2
    return L.bufs


@scenario
def learner_window_play(c):
    return _play_twice(c, "window")


@scenario
def learner_window_greedy_play(c):
    return _play_twice(c, "window_greedy")


@scenario
def learner_playout_play_targets(c):
    _play_twice(c, "playout")


@scenario
def learner_playout_targets(c):
    L = _learner(c, "playout")
    L.play()
    c.forget()
    c.a("L.roots", L.roots), c.a("L.target", L.target), c.a("L.weight", L.weight)
    ret = L.targets()
    c.a("L.result", L.result)
    return ret


@scenario
def learner_lookahead_play(c):
    _play_twice(c, "lookahead")


@scenario
def learner_lookahead_targets(c):
    L = _learner(c, "lookahead")
    c.a("L.roots", L.roots), c.a("L.target", L.target), c.a("L.weight", L.weight)
    return L.targets()


def _trim(out):
    """A player's step tuple without the env's own outputs."""
    return out[4], out[5], out[6], out[7]


@scenario
def player_plain_module(c):
    p = value_play.ValuePlayer(c.env, lambda feat: feat.sum(1), perspective="mover")
    assert not p.fused
    return _trim(p.step())


@scenario
def player_fused_cap(c):
    c.temporaries = True
    p = value_play.ValuePlayer(c.env, c.net, cap=5)
    assert p.fused and p.plies == 1
    return _trim(p.step(epsilon=0.5, tag=3, seed=9))


@scenario
def player_fused_neither(c):
    return _trim(value_play.ValuePlayer(c.env, c.net, perspective="mover").step())


@scenario
def player_lookahead(c):
    p = value_play.LookaheadPlayer(c.env, c.net, cap=5)
    assert p.plies == 2 and p.top is None
    return _trim(p.step())


@scenario
def player_lookahead_top(c):
    c.temporaries = True
    return _trim(value_play.LookaheadPlayer(c.env, c.net, cap=5, top=2).step())


@scenario
def player_playout(c):
    c.temporaries = True
    p = value_play.PlayoutPlayer(c.env, c.net, k=2, trials=3, max_plies=5, playout_net=c.other, truncated=True,
                                 cap=5, seed=100)
    out = p.step()
    assert p._ply == 12
    res = out[4].pop("playout")
    assert isinstance(res, PlayoutResult) and res.leaf is not None
    return _trim(out)


@scenario
def match(c):
    c.temporaries = True
    f = value_play.play_turn_match if c.env.full else value_play.play_match
    res = f(c.env, c.net, None, 2, epsilon=0.25, seed=3)
    assert set(res) == {"games", "points_a", "points_b", "by_colour"}


@scenario
def league(c):
    c.temporaries = True
    res = value_play.play_league(c.env, [c.net, c.other], 2, pairs=[(0, 1), (1, -1)], seed=3)
    assert res["white"].tolist() == [0, 1, 0] and res["black"].tolist() == [1, -1, 1]


REF2_ONLY = {"player_two_plies"}


@scenario
def player_two_plies(c):  # ValuePlayer(plies=2) is rules="ref2" only
    return _trim(value_play.ValuePlayer(c.env, c.net, cap=1, plies=2).step())


def trace(rules, name):
    c = Ctx(rules)
    ret = S[name](c)
    return describe(c, ret)


def cases():
    return [(r, n) for n in S for r in RULES if not (r == "full4" and n in REF2_ONLY)]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_scenarios(golden):
    assert sorted(golden) == sorted(f"{r}/{n}" for r, n in cases())


@pytest.mark.parametrize("rules,name", cases())
def test_calls(golden, rules, name):
    want, got = golden[f"{rules}/{name}"], trace(rules, name)
    assert got["calls"] == want["calls"]
    assert got["ret"] == want["ret"]
    # the env holds at least what it held: the C side reads these after the call returns
    assert set(want["keep"]) <= set(got["keep"]), (want["keep"], got["keep"])


def test_neither_is_two_calls_and_one_item(monkeypatch):
    """cap None: the sizing call, one .item(), the call at the size read."""
    items = []
    real = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "item", lambda self: items.append(1) or real(self))
    for rules in RULES:
        for key, args in (("expand", ()), ("scored", (Net("n"),)), ("look", (Net("n"),)), ("rec", (Net("n"),))):
            del items[:]
            c = Ctx(rules)
            ret = c.call(key, *args)
            aft = ret if key == "expand" else ret[0]
            assert len(items) == 1 and len(c.env.handle.calls) == 2 and aft.cap == TOTAL
            del items[:]
            c = Ctx(rules)
            c.call(key, *args, cap=5)
            assert not items and len(c.env.handle.calls) == 1


# ------------------------------------------------------------------- errors
META = torch.device("meta")
I32, F32, U8 = "torch.int32", "torch.float32", "torch.uint8"


def raises(exc, text, f, *args, **kw):
    with pytest.raises(exc) as e:
        f(*args, **kw)
    assert type(e.value) is exc and str(e.value) == text


def _row(text, dt):
    return f"{text} must be a contiguous {dt} device tensor of at least cap rows"


@pytest.mark.parametrize("rules", RULES)
def test_rule_set_guards(rules):
    c, other = Ctx(rules), M["full4" if rules == "ref2" else "ref2"]
    want = "ref2" if rules == "full4" else "full4"
    for key in ("expand", "scored", "look", "rec", "roll", "league"):
        name = other[key]
        raises(ValueError, f'{name}() is rules="{want}" only', getattr(c.env, name), *([None] * 4))
    if rules == "ref2":
        raises(ValueError, 'pick_turn() is rules="full4" only', c.env.pick_turn, None, None)
        raises(ValueError, 'play_turn_match() is rules="full4" only', value_play.play_turn_match, c.env, c.net, None, 1)
    else:
        raises(ValueError, 'play_match() is rules="ref2" only', value_play.play_match, c.env, c.net, None, 1)
        raises(ValueError, 'plies=2 is rules="ref2" only', value_play.ValuePlayer, c.env, c.net, plies=2)
    assert not c.env.handle.calls


@pytest.mark.parametrize("rules", RULES)
def test_expansion_errors(rules):
    c = Ctx(rules)
    m, f, dt = c.m, c.m["field"], str(c.m["dtype"])
    net, far = c.net, Net("far", device=META)
    bad = {"offsets": (torch.zeros(B, dtype=torch.int32), I32), "row_env": (torch.zeros(5, dtype=torch.int64), I32),
           f: (torch.zeros((5, 3), dtype=m["dtype"]), dt), "feat": (torch.zeros((5, 198), device=META), F32),
           "obs": (torch.zeros((10, 24), dtype=torch.int32)[::2], I32), "reward": (torch.zeros(4, dtype=torch.int8), "torch.int8")}
    for name, (a, text) in bad.items():
        out = c.aft(5, feat=True, obs=True)._replace(**{name: a})
        raises(ValueError, _row(f"out.{name}", text), c.call, "expand", out=out)
        if name not in ("feat", "obs"):
            raises(ValueError, _row(f"out {name}", text), c.call, "scored", net, out=out)
            raises(ValueError, _row(f"out {name}", text), c.call, "look", net, out=(out, torch.zeros(5)))
            raises(ValueError, _row(f"out {name}", text), c.call, "rec", net, out=(out, torch.zeros(5), rec(5)))
    good = c.aft(5)
    # the first bad array in the tuple's order is the one named
    raises(ValueError, _row("out.row_env", I32), c.call, "expand",
           out=good._replace(row_env=torch.zeros(4, dtype=torch.int32), reward=torch.zeros(4, dtype=torch.int8)))
    raises(ValueError, _row("out values", F32), c.call, "scored", net, out=(good, torch.zeros(4)))
    raises(ValueError, _row("out values", F32), c.call, "scored", net, out=(good, torch.zeros(5, dtype=torch.float64)))
    raises(ValueError, _row("out reward", "torch.int8"), c.call, "scored", net,
           out=(good._replace(reward=torch.zeros(4, dtype=torch.int8)), torch.zeros(4)))
    raises(ValueError, _row("out values", F32), c.call, "rec", net, out=(good, None, rec(5)))
    raises(ValueError, _row("out values", F32), c.call, "rec", net, out=(good, torch.zeros(4), rec(4)))
    raises(ValueError, _row("out records", I32), c.call, "rec", net, out=(good, torch.zeros(5), None))
    raises(ValueError, _row("out records", I32), c.call, "rec", None, out=(good, None, rec(4)))
    raises(ValueError, _row("out records", I32), c.call, "rec", None, out=(good, None, torch.zeros((5, 7), dtype=torch.int32)))
    # rows a records call may leave out; a values tensor is checked when given, net or none
    c.call("rec", None, out=(good._replace(row_env=None, reward=None, **{f: None}), None, rec(5)))
    raises(ValueError, _row("out values", F32), c.call, "rec", None, out=(good, torch.zeros(1), rec(5)))
    for key, args in (("expand", ()), ("scored", (net,)), ("look", (net,)), ("rec", (net,))):
        raises(ValueError, "cap must be >= 0", c.call, key, *args, cap=-1)
        out = good if key == "expand" else (good, torch.zeros(5)) + ((rec(5),) if key == "rec" else ())
        raises(ValueError, "cap must be >= 0", c.call, key, *args, cap=-1, out=out)
    # with out, a records call checks cap before its arrays; the others check their arrays first
    short = good._replace(offsets=torch.zeros(B, dtype=torch.int32))
    raises(ValueError, "cap must be >= 0", c.call, "rec", net, cap=-1, out=(short, torch.zeros(5), rec(5)))
    raises(ValueError, _row("out.offsets", I32), c.call, "expand", cap=-1, out=short)
    raises(ValueError, _row("out offsets", I32), c.call, "scored", net, cap=-1, out=(short, torch.zeros(5)))
    persp = "perspective must be one of ('mover', 'white')"
    raises(ValueError, persp, c.call, "scored", object(), perspective="black")
    raises(TypeError, "net must be a gym_narde.value_net.ValueMLP", c.call, "scored", object(), cap=-1)
    raises(ValueError, "the net must live on the env's device", c.call, "scored", far, cap=-1)
    raises(TypeError, "net must be a gym_narde.value_net.ValueMLP", c.call, "look", object(), cap=-1)
    raises(ValueError, "the net must live on the env's device", c.call, "look", far, cap=-1)
    raises(TypeError, "net must be a gym_narde.value_net.ValueMLP or None", c.call, "rec", object(), cap=-1)
    raises(ValueError, "the net must live on the env's device", c.call, "rec", far, cap=-1)
    # a net's struct() is made before its device is looked at (the tables look first: test_rollout_errors)
    for key in ("scored", "look", "rec"):
        raises(ValueError, "no struct", c.call, key, Unpacked(), cap=-1)
    raises(ValueError, "expected shape (3, 2), got (3, 3)", c.call, "scored", net, torch.zeros((B, 3)), cap=-1)
    raises(ValueError, "expected shape (3, 2), got (3, 3)", c.call, "expand", torch.zeros((B, 3)), cap=-1)


@pytest.mark.parametrize("rules", RULES)
def test_pick_errors(rules):
    c = Ctx(rules)
    e, aft, v = c.env, c.aft(5), torch.zeros(5)
    sel, res = torch.zeros((B, 2), dtype=torch.int32), _result(c)
    persp = "perspective must be one of ('mover', 'white')"
    vals = "values must be float32, one per afterstate row (at least 5), on the env's device"
    together = "epsilon and tag go together"
    raises(ValueError, persp, c.call, "pick", aft, None, "black", 0.5)
    raises(ValueError, vals, c.call, "pick", aft, torch.zeros(4), "white", 0.5)
    raises(ValueError, vals, c.call, "pick", aft, torch.zeros((5, 2)))
    raises(ValueError, vals, c.call, "pick", aft, torch.zeros(5, dtype=torch.float64))
    raises(ValueError, vals, c.call, "pick", aft, torch.zeros(5, device=META))
    raises(ValueError, vals, c.call, "pick", aft, torch.zeros(1).expand(5))
    raises(ValueError, together, c.call, "pick", aft, v, epsilon=0.5)
    raises(ValueError, together, c.call, "pick", c.aft(0), torch.zeros(0), tag=1)
    # top_rows
    raises(ValueError, persp, e.top_rows, aft, v, 0, perspective="black")
    raises(ValueError, "k must be in 1 .. 64", e.top_rows, aft, None, 0)
    raises(ValueError, "k must be in 1 .. 64", e.top_rows, aft, None, 65)
    raises(ValueError, vals, e.top_rows, aft, torch.zeros(4), 1, records=rec(4))
    for bad in (rec(4), rec(5).long(), torch.zeros((5, 7), dtype=torch.int32), rec(10)[::2], rec(5).to(META)):
        raises(ValueError, "records must be a contiguous (>= cap, 8) int32 device tensor", e.top_rows, aft, v, 1, bad)
    # pick_playout: the leaf, sel, the sums, the leaf's shape, the values -- in that order
    leaf = "leaf=True needs the playouts' leaf values (playout(leaf=True))"
    sel_text = "sel must be top_rows()' (B, k) int32 tensor"
    raises(ValueError, leaf, e.pick_playout, aft, v, None, _result(c, leaf=False), leaf=True)
    raises(ValueError, leaf, e.pick_playout, aft, v, None, (res.sums, 3), leaf=True)
    for bad in (sel[0], sel[:2], sel.long(), torch.zeros((B, 4), dtype=torch.int32)[:, ::2]):
        raises(ValueError, sel_text, e.pick_playout, aft, v, bad, (None, 3))
    for bad in (res.sums[:4], res.sums.long(), torch.zeros((B * 2, 8), dtype=torch.int32)[:, ::2], res.sums.to(META)):
        raises(ValueError, "result must hold the sums of B * k roots", e.pick_playout, aft, None, sel, (bad, 3, None))
    for bad in (res.leaf[:, :2], res.leaf.double(), torch.zeros((B * 2, 6))[:, ::2]):
        raises(ValueError, "leaf must be (B * k, trials) float32", e.pick_playout, aft, None, sel, (res.sums, 3, bad), True)
    raises(ValueError, vals, e.pick_playout, aft, torch.zeros(4), sel, res)
    e.pick_playout(aft, v, sel, (res.sums, 3, res.leaf[:, :2]))  # a leaf the call does not use is not looked at
    # pick_slots: sel, k, the scores, the values
    score = "slot_score must be a contiguous (B, k) or (B * k,) float32 device tensor"
    for bad in (None, sel[0], sel[:2], sel.long(), torch.zeros((B, 4), dtype=torch.int32)[:, ::2], sel.to(META)):
        raises(ValueError, sel_text, e.pick_slots, aft, v, bad, None)
    raises(ValueError, "k must be in 1 .. 64", e.pick_slots, aft, v, torch.zeros((B, 65), dtype=torch.int32), None)
    raises(ValueError, "k must be in 1 .. 64", e.pick_slots, aft, v, torch.zeros((B, 0), dtype=torch.int32), None)
    for bad in (None, torch.zeros((B, 2), dtype=torch.float64), torch.zeros((B, 2), device=META), torch.zeros((B, 4))[:, ::2],
                torch.zeros((B, 3)), torch.zeros((2, B)), torch.zeros((B, 2, 1))):
        raises(ValueError, score, e.pick_slots, aft, None, sel, bad)
    raises(ValueError, vals, e.pick_slots, aft, torch.zeros(4), sel, torch.zeros((B, 2)))
    # lookahead_records: the records, the net, out
    text = "records must be a contiguous (n, 8) int32 device tensor of records, n >= 1"
    for bad in (None, rec(4).long(), rec(4).to(META), rec(8)[::2], rec(4)[0], rec(4)[:, :7], rec(4)[:0]):
        raises(ValueError, text, e.lookahead_records, bad, object())
    raises(TypeError, "net must be a gym_narde.value_net.ValueMLP", e.lookahead_records, rec(4), object(), out=0)
    raises(ValueError, "the net must live on the env's device", e.lookahead_records, rec(4), Net("far", device=META), out=0)
    for bad in (torch.zeros(5), torch.zeros(4, dtype=torch.float64), torch.zeros(4, device=META), torch.zeros(8)[::2]):
        raises(ValueError, "out must be a contiguous (n,) float32 device tensor", e.lookahead_records, rec(4), c.net, bad)
    # playout_targets: the leaf, the sums, the leaf's shape, the roots
    sums = torch.zeros((B, 4), dtype=torch.int32)
    raises(ValueError, leaf, e.playout_targets, (None, 3), leaf=True)
    for bad in (sums[0], sums[:, :3], sums[:0], sums.long(), torch.zeros((B, 8), dtype=torch.int32)[:, ::2], sums.to(META)):
        raises(ValueError, "result must hold (N, 4) int32 sums on this device", e.playout_targets, (bad, 3, None))
    for bad in (torch.zeros((B, 2)), torch.zeros((B, 3), dtype=torch.float64), torch.zeros((B, 6))[:, ::2]):
        raises(ValueError, "leaf must be (N, trials) float32", e.playout_targets, (sums, 3, bad), torch.zeros(1), True)
    for bad in (rec(2), rec(B).long(), rec(2 * B)[::2], rec(B).to(META)):
        raises(ValueError, "roots must be the playouts' contiguous (N, 8) int32 records", e.playout_targets, (sums, 3), bad)
    assert len(e.handle.calls) == 1  # (the one pick_playout above)


@pytest.mark.parametrize("rules", RULES)
def test_rollout_errors(rules):
    c = Ctx(rules)
    e, net, far = c.env, c.net, Net("far", device=META)
    plies, none = "plies must be >= 1", "a net for at least one colour (random play on both sides is selfplay())"
    together = "epsilon and tag go together"
    typ, dev = "net must be a gym_narde.value_net.ValueMLP", "the net must live on the env's device"
    piece = ("scratch must be a contiguous uint8 device tensor of at least one piece (83536 bytes; "
             "turn_value_rollout_scratch())")
    col, shp = ("play", ", 4, 2") if e.full else ("actions", ", 2")
    # value_rollout: plies, the nets (white before black), the explore pair, the buffers, the scratch
    raises(ValueError, plies, c.call, "roll", 0, None, None)
    raises(ValueError, none, c.call, "roll", 1, None, epsilon=0.5)
    raises(ValueError, none, c.call, "roll", 1, None, None, epsilon=0.5)
    raises(TypeError, typ, c.call, "roll", 1, object(), far, epsilon=0.5)
    raises(ValueError, dev, c.call, "roll", 1, far, object(), epsilon=0.5)
    raises(TypeError, typ, c.call, "roll", 1, None, object())
    raises(ValueError, together, c.call, "roll", 1, net, epsilon=0.5, bufs={"dice": 0})
    raises(ValueError, together, c.call, "roll", 1, net, tag=2)
    buf = {"dice": ("uint8", ", 2", (2, B, 2), torch.uint8), col: (str(c.m["dtype"])[6:], shp, (2, B) + c.m["shape"], c.m["dtype"]),
           "value": ("float32", "", (2, B), torch.float32), "reward": ("int32", "", (2, B), torch.int32),
           "terminated": ("uint8", "", (2, B), torch.uint8), "truncated": ("uint8", "", (2, B), torch.uint8),
           "records": ("int32", ", 8", (2, B, 8), torch.int32)}
    scratch = dict(scratch=torch.zeros(3)) if e.full else {}
    table, w = torch.zeros(128, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32)
    for name, (dt, tail, shape, dtype) in buf.items():
        text = f"bufs['{name}'] must be a contiguous {dt} device tensor of shape (>= 2, 3{tail})"
        for bad in (torch.zeros((1,) + shape[1:], dtype=dtype), torch.zeros(shape, dtype=torch.float64),
                    torch.zeros(shape, dtype=dtype, device=META), torch.zeros(shape + (2,), dtype=dtype)[..., 0],
                    torch.zeros(shape[:1] + (4,) + shape[2:], dtype=dtype), torch.zeros(shape + (1,), dtype=dtype)):
            raises(ValueError, text, c.call, "roll", 2, net, bufs={name: bad}, **scratch)
            raises(ValueError, text, c.call, "league", 2, table, w, w, bufs={name: bad}, **scratch)
    if e.full:
        for bad in (torch.zeros(83536), torch.zeros(83535, dtype=torch.uint8), torch.zeros(2 * 83536, dtype=torch.uint8)[::2],
                    torch.zeros(83536, dtype=torch.uint8, device=META)):
            raises(ValueError, piece, e.turn_value_rollout, 1, net, scratch=bad)
            raises(ValueError, piece, e.turn_value_rollout_league, 1, table, w, w, scratch=bad)
            raises(ValueError, piece, e.playout, rec(1), 1, net, scratch=bad)
        raises(ValueError, "waves must be >= 1", e.turn_value_rollout_scratch, 0)
    # the league launches: plies, the table, white, black, the explore pair, the buffers
    tab = "table must be net_table()'s uint8 tensor on the env's device"
    raises(ValueError, plies, c.call, "league", 0, None, None, None)
    for bad in (None, torch.zeros(128), torch.zeros(128, dtype=torch.uint8, device=META), torch.zeros(256, dtype=torch.uint8)[::2],
                torch.zeros((2, 64), dtype=torch.uint8), torch.zeros(100, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8),
                torch.zeros(65 * 64, dtype=torch.uint8), torch.zeros(192, dtype=torch.uint8)[8:136]):
        raises(ValueError, tab, c.call, "league", 1, bad, None, None)
    for bad in (None, w.long(), w.to(META), torch.zeros(2 * B, dtype=torch.int32)[::2], torch.zeros(B + 1, dtype=torch.int32)):
        raises(ValueError, "white must be a contiguous int32 device tensor of shape (3,)", c.call, "league", 1, table, bad, bad)
        raises(ValueError, "black must be a contiguous int32 device tensor of shape (3,)", c.call, "league", 1, table, w, bad,
               epsilon=0.5)
    raises(ValueError, together, c.call, "league", 1, table, w, w, epsilon=0.5, bufs={"dice": 0})
    # net_table: the count, the nets in order (a net's type before its device), out
    raises(ValueError, "a table holds 1 .. 64 nets, not 0", e.net_table, [])
    raises(ValueError, "a table holds 1 .. 64 nets, not 65", e.net_table, [object()] * 65)
    raises(TypeError, "nets[1] must be a gym_narde.value_net.ValueMLP", e.net_table, [net, object(), far])
    raises(ValueError, "nets[0] must live on the env's device", e.net_table, [far, object()])
    raises(ValueError, "nets[0] must live on the env's device", e.net_table, [Unpacked()])
    raises(ValueError, "no struct", c.call, "roll", 1, Unpacked())
    raises(ValueError, "no struct", e.playout, rec(1), 1, None, Unpacked())
    raises(ValueError, "no struct", e.lookahead_records, rec(1), Unpacked())
    out = "out must be a contiguous, 16-B aligned uint8 device tensor of at least 128 bytes"
    for bad in (torch.zeros(128), torch.zeros(128, dtype=torch.uint8, device=META), torch.zeros(256, dtype=torch.uint8)[::2],
                torch.zeros((2, 64), dtype=torch.uint8), torch.zeros(127, dtype=torch.uint8), torch.zeros(192, dtype=torch.uint8)[8:]):
        raises(ValueError, out, e.net_table, [net, net], out=bad)
    # playout: the roots, the counts, the nets, out, the scratch
    roots = "roots must be a contiguous (N, 8) int32 device tensor of records, or a get_state() dict"
    for bad in (None, rec(2).long(), rec(2).to(META), rec(4)[::2], rec(2)[0], rec(2)[:, :7], rec(2)[:0]):
        raises(ValueError, roots, e.playout, bad, 0, None, None)
    raises(ValueError, "trials and max_plies must be >= 1", e.playout, rec(2), 0, None, None)
    raises(ValueError, "trials and max_plies must be >= 1", e.playout, rec(2), 1, None, None, max_plies=0)
    raises(ValueError, none, e.playout, rec(2), 1, None, None, out=0)
    raises(TypeError, typ, e.playout, rec(2), 1, object(), out=0)
    raises(ValueError, dev, e.playout, rec(2), 1, net, far, out=0)
    res = "out must be a PlayoutResult of the same roots and trials on this device"
    for bad in (PlayoutResult(torch.zeros((3, 4), dtype=torch.int32), 2), PlayoutResult(torch.zeros((2, 4), dtype=torch.int32), 3),
                PlayoutResult(torch.zeros((2, 4), dtype=torch.int32, device=META), 2)):
        raises(ValueError, res, e.playout, rec(2), 2, net, out=bad, scratch=0)
    assert not e.handle.calls


def test_caller_errors():
    c, thing = Ctx("ref2"), types.SimpleNamespace(struct=0)  # (struct alone is not a ValueMLP to these)
    e = c.env
    for name in ("WindowTDLambdaLearner", "PlayoutTargetLearner", "LookaheadTargetLearner"):
        args = (0.1, 0.5, 2) if name == "WindowTDLambdaLearner" else (0.1, 2, 3)[:3 if name[0] == "P" else 2]
        raises(TypeError, f"{name} needs a gym_narde.value_net.ValueMLP", getattr(td, name), Env(autoreset=False), thing, *args)
        raises(ValueError, f"{name} needs an env with autoreset=True", getattr(td, name), Env(autoreset=False),
               Net("far", device=META), *args)
        raises(ValueError, "the net is on meta, the env on cpu", getattr(td, name), e, Net("far", device=META), *args)
    raises(ValueError, "lam must be in [0, 1]", td.WindowTDLambdaLearner, e, c.net, 0.1, 1.5, 0)
    raises(ValueError, "plies must be >= 1", td.WindowTDLambdaLearner, e, c.net, 0.1, 0.5, 0)
    raises(TypeError, "ValueFitter needs a gym_narde.value_net.ValueMLP", td.ValueFitter, e, thing, 0)
    raises(ValueError, "the net is on meta, the env on cpu", td.ValueFitter, e, Net("far", device=META), 0)
    raises(TypeError, "TDLambdaLearner needs a gym_narde.value_net.ValueMLP", td.TDLambdaLearner, Env(autoreset=False), thing, 0.1, 2)
    raises(TypeError, "ValueSGD needs a gym_narde.value_net.ValueMLP", td.ValueSGD, thing, 0.1)
    raises(TypeError, "ValueAdam needs a gym_narde.value_net.ValueMLP", td.ValueAdam, thing, 0.1)
    raises(TypeError, "fused=True needs a gym_narde.value_net.ValueMLP", value_play.ValuePlayer, e, thing, fused=True)
    raises(TypeError, "plies=2 needs a gym_narde.value_net.ValueMLP", value_play.ValuePlayer, e, thing, plies=2)
    raises(TypeError, "LookaheadPlayer needs a gym_narde.value_net.ValueMLP", value_play.LookaheadPlayer, e, thing)
    raises(TypeError, "PlayoutPlayer needs a gym_narde.value_net.ValueMLP", value_play.PlayoutPlayer, e, thing)
    assert not value_play.ValuePlayer(e, thing).fused
    raises(TypeError, "nets[1] must be a gym_narde.value_net.ValueMLP", value_play.play_league, e, [c.net, thing], 1)
    raises(ValueError, "nets[0] must live on the env's device", value_play.play_league, e, [Net("far", device=META), thing], 1)
    raises(ValueError, "plies, trials, every and max_plies must be >= 1", td.PlayoutTargetLearner, e, c.net, 0.1, 2, 0)
    raises(ValueError, "plies, trials, every and max_plies must be >= 1", td.PlayoutTargetLearner, e, c.net, 0.1, 2, 3,
           max_plies=0)
    raises(ValueError, "plies and every must be >= 1", td.LookaheadTargetLearner, e, c.net, 0.1, 2, every=0)
    raises(ValueError, "perspective must be one of ('mover', 'white')", value_play.ValuePlayer, e, c.net, "black")
    raises(ValueError, "cap is the fused path's", value_play.ValuePlayer, e, thing, cap=5)
    raises(ValueError, "plies must be 1 or 2", value_play.ValuePlayer, e, c.net, plies=3)
    raises(ValueError, "plies=2 is the fused path's", value_play.ValuePlayer, e, c.net, fused=False, plies=2)
    raises(ValueError, 'plies=2 needs perspective "white"', value_play.ValuePlayer, e, c.net, "mover", plies=2)
    raises(TypeError, "top must be None or an int", value_play.LookaheadPlayer, e, c.net, top=True)
    raises(TypeError, "top must be None or an int", value_play.LookaheadPlayer, e, c.net, top=2.0)
    raises(ValueError, "top must be in 1 .. 64", value_play.LookaheadPlayer, e, c.net, top=0)
    raises(ValueError, "top must be in 1 .. 64", value_play.LookaheadPlayer, e, c.net, top=65)
    raises(ValueError, "the pruned search (top) plays greedily: no epsilon",
           value_play.LookaheadPlayer(e, c.net, top=1).step, epsilon=0.5)
    raises(ValueError, "net_a is the net under test; pass None as net_b for the random baseline", value_play.play_match,
           e, None, c.net, 1)
    assert not e.handle.calls


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_vector_calls_cpu.py --record")
    with open(GOLDEN, "w") as f:
        json.dump({f"{r}/{n}": trace(r, n) for r, n in cases()}, f, indent=1, sort_keys=True)
        f.write("\n")
