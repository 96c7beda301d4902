"""What the two afterstate GPU test files (test_gpu_afterstates.py: REF2,
test_gpu_turn_afterstates.py: FULL4) share: the env on given states, the
row-for-row comparison, the pick's torch reference and the scored ply.
"""
import numpy as np
import torch

np_ = lambda t: t.cpu().numpy()  # noqa: E731


def _env(st, rules="ref2", seed=3, autoreset=False, **kw):
    """A VecNardeEnv set to the states st = (board, off, first_turn, player, ...)."""
    from gym_narde.vector import VecNardeEnv

    env = VecNardeEnv(len(st[3]), device="cuda:0", seed=seed, autoreset=autoreset, rules=rules, **kw)
    env.set_state(st[0], st[1], st[2], st[3])
    return env


def _equal(aft, want, rows=None, action="codes"):
    n = int(want["offsets"][-1]) if rows is None else rows
    assert np.array_equal(np_(aft.offsets), want["offsets"])
    assert np.array_equal(np_(aft.row_env)[:n], want["row_env"][:n])
    assert np.array_equal(np_(getattr(aft, action))[:n], want[action][:n])
    assert np.array_equal(np_(aft.reward)[:n], want["reward"][:n])
    assert np.array_equal(np_(aft.feat)[:n].view(np.uint32), want["feat"][:n].view(np.uint32))
    if aft.obs is not None:
        assert np.array_equal(np_(aft.obs)[:n], want["obs"][:n].astype(np.int32))


def _pick_ref(offsets, cap, values, black, perspective):
    """torch.max / torch.min over each env's rows (below cap): (row, NaN as
    torch takes it, the first of equal values)."""
    v = torch.as_tensor(values)
    rows = np.full(len(offsets) - 1, -1, np.int32)
    for e in range(len(offsets) - 1):
        r0, r1 = int(offsets[e]), min(int(offsets[e + 1]), cap)
        if r1 <= r0:
            continue
        seg = v[r0:r1]
        smallest = perspective == "white" and black[e]
        # first extremum: torch.min / max(dim) on the CPU return it
        k = int((torch.min(seg, 0) if smallest else torch.max(seg, 0)).indices)
        ext = seg[k]
        same = torch.isnan(seg) if torch.isnan(ext) else seg == ext
        rows[e] = r0 + int(torch.nonzero(same)[0])
    return rows


def _check_pick(env, aft, values, black, perspective, actions, **kw):
    """The env's pick against _pick_ref; actions: the reference rows' action
    column ("no row": 0 for REF2 codes, -1 for FULL4 plays)."""
    pick, none = (env.pick_turn, -1) if env.full else (env.pick_afterstate, 0)
    got, row = pick(aft, values, perspective=perspective, **kw)
    want = _pick_ref(np_(aft.offsets), aft.cap, np_(values), black, perspective)
    assert np.array_equal(np_(row), want)
    has = (want >= 0).reshape((-1,) + (1,) * (actions.ndim - 1))
    assert np.array_equal(np_(got), np.where(has, actions[np.maximum(want, 0)], none))
    return want


def _scored_ply(env, out, score):
    """One ply into preallocated rows: expand, values = score(feat), pick, step."""
    expand, pick = (env.turn_afterstates, env.pick_turn) if env.full else (env.afterstates, env.pick_afterstate)
    aft = expand(out=out)
    with torch.no_grad():
        values = score(aft.feat)
    actions, row = pick(aft, values, perspective="white")
    env.step(actions)
    return actions, row
