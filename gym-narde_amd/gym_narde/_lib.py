"""ctypes binding of libnarde.so (include/narde.h).

The product path has exactly one implementation: the HIP kernels in
libnarde.so.  There is no CPU fallback -- if the library or a GPU is missing,
every entry point raises NardeLibraryError.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NARDE_LIB", os.path.join(HERE, "libnarde.so"))

OK = 0
OFF = 24
MAX_MOVES = 64
TD_SLAB = 64  # NARDE_TD_SLAB
TD_WINDOW_SLAB = 128  # NARDE_TD_WINDOW_SLAB
TOTAL_ROWS = 64  # NARDE_TOTAL_ROWS


def wg_rows(num_envs):
    """NARDE_WG_ROWS: rows of narde_rollout_timed's per-workgroup totals."""
    return (int(num_envs) + 255) // 256


def td_scratch_floats(num_envs, hidden):
    """NARDE_TD_SCRATCH_FLOATS: narde_value_td_apply's scratch."""
    b = int(num_envs)
    return (b + 3) // 4 * 4 + (b + TD_SLAB - 1) // TD_SLAB * (200 * int(hidden) + 4)


def td_window_scratch_floats(num_envs, plies, hidden):
    """NARDE_TD_WINDOW_SCRATCH_FLOATS: narde_value_td_window's scratch."""
    b, k = int(num_envs), int(plies)
    return (((k + 1) * b + 3) // 4 * 4 + (k * b + 3) // 4 * 4
            + (k * b + TD_WINDOW_SLAB - 1) // TD_WINDOW_SLAB * (200 * int(hidden) + 4))


VALUE_FIT_SLAB = TD_WINDOW_SLAB  # NARDE_VALUE_FIT_SLAB


def value_fit_scratch_floats(n, hidden):
    """NARDE_VALUE_FIT_SCRATCH_FLOATS: narde_value_fit's scratch (a partial
    row and two doubles a slab)."""
    return (int(n) + VALUE_FIT_SLAB - 1) // VALUE_FIT_SLAB * (200 * int(hidden) + 4 + 4)


def lookahead_scratch_bytes(cap):
    """NARDE_LOOKAHEAD_SCRATCH_BYTES: narde_afterstates_lookahead's scratch."""
    return 32 * int(cap)


def turn_lookahead_scratch_bytes(cap):
    """NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES: narde_turn_afterstates_lookahead's scratch."""
    return 128 * int(cap)


def turn_rollout_scratch_bytes(waves):
    """NARDE_TURN_ROLLOUT_SCRATCH_BYTES: narde_turn_value_rollout's scratch, a piece a wave."""
    return 83536 * int(waves)


LEAGUE_NETS_MAX = 64  # NARDE_LEAGUE_NETS_MAX


def league_table_bytes(n_nets):
    """NARDE_LEAGUE_TABLE_BYTES: narde_net_table's table, an entry a net."""
    return 64 * int(n_nets)


PLAYOUT_COMMON_DICE = 1  # NARDE_PLAYOUT_COMMON_DICE
TOPK_MAX = 64  # NARDE_TOPK_MAX
RECORD_NONE_WORD6 = 0xFF  # NARDE_RECORD_NONE_WORD6

DICE_ALL36 = 0
DICE_NODOUBLES = 1

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int
_u32 = ctypes.c_uint32
_u64 = ctypes.c_uint64



class ValueMlp(ctypes.Structure):
    """narde_value_mlp: device pointers of a 198 -> hidden -> 1 value net."""
    _fields_ = [("w1t", _vp), ("ld_w1t", _i64), ("b1", _vp), ("w2", _vp), ("b2", _vp),
                ("hidden", ctypes.c_int32), ("hidden_act", ctypes.c_int32), ("out_act", ctypes.c_int32)]


class ValueMlpTrain(ctypes.Structure):
    """narde_value_mlp_train: ValueMlp's fields, writable, and the optional
    row-major mirror of the first layer."""
    _fields_ = ValueMlp._fields_ + [("w1", _vp), ("ld_w1", _i64)]


# name -> (restype, argtypes); mirrors include/narde.h one to one
SIGNATURES = {
    "narde_version": (_i32, []),
    "narde_last_error": (ctypes.c_char_p, []),
    "narde_create": (_i32, [_i32, _i64, _i64, _u64, _i32, _i32, ctypes.POINTER(_vp)]),
    "narde_destroy": (_i32, [_vp]),
    "narde_num_envs": (_i64, [_vp]),
    "narde_get_ply": (_i32, [_vp, ctypes.POINTER(_u32)]),
    "narde_set_ply": (_i32, [_vp, _u32]),
    "narde_reset": (_i32, [_vp, _vp, _vp, _i32, _vp]),
    "narde_set_state": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_get_state": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_peek_dice": (_i32, [_vp, _vp, _vp]),
    "narde_legal_moves": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "narde_rollout": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_selfplay": (_i32, [_vp, _i32, _vp]),
    "narde_step_full": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "narde_rollout_full": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_selfplay_full": (_i32, [_vp, _i32, _vp]),
    "narde_rollout_timed": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_rollout_plan_create": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_rollout_plan_launch": (_i32, [_vp]),
    "narde_rollout_plan_destroy": (_i32, [_vp]),
    "narde_timing_event_create": (_i32, [_i32, ctypes.c_uint, ctypes.POINTER(_vp)]),
    "narde_timing_event_destroy": (_i32, [_vp]),
    "narde_timing_event_elapsed_ms": (_i32, [_vp, _vp, ctypes.POINTER(ctypes.c_float)]),
    "narde_legal_full": (_i32, [_vp, _vp, _vp, _vp]),
    "narde_get_stats": (_i32, [_vp, _vp, _vp]),
    "narde_get_totals": (_i32, [_vp, _vp, _vp]),
    "narde_apply_moves": (_i32, [_vp, _vp, _vp, _vp]),
    "narde_observe": (_i32, [_vp, _vp, _vp, _vp]),
    "narde_legal_mask576": (_i32, [_vp, _vp, _vp]),
    "narde_legal_mask576_move2": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "narde_play_set": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "narde_act_masks": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "narde_explore_plays": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _i64, _vp]),
    "narde_afterstates": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_afterstate_pick": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "narde_turn_afterstates": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_turn_pick": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "narde_afterstates_scored": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(ValueMlp), _i32, _vp, _vp]),
    "narde_turn_afterstates_scored": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(ValueMlp), _i32, _vp,
                                             _vp]),
    "narde_afterstates_lookahead": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(ValueMlp), _i32, _vp, _vp,
                                           _i64, _vp]),
    "narde_value_rollout": (_i32, [_vp, _i32, ctypes.POINTER(ValueMlp), ctypes.POINTER(ValueMlp), _vp, _u64, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_value_rollout_records": (_i32, [_vp, _i32, ctypes.POINTER(ValueMlp), ctypes.POINTER(ValueMlp), _vp, _u64, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_turn_afterstates_lookahead": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(ValueMlp), _i32, _vp,
                                                _vp, _i64, _vp]),
    "narde_turn_value_rollout_waves": (_i32, [_vp, _vp]),
    "narde_turn_value_rollout": (_i32, [_vp, _i32, ctypes.POINTER(ValueMlp), ctypes.POINTER(ValueMlp), _vp, _u64, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "narde_turn_value_rollout_records": (_i32, [_vp, _i32, ctypes.POINTER(ValueMlp), ctypes.POINTER(ValueMlp), _vp, _u64,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "narde_net_table": (_i32, [_i32, _i32, ctypes.POINTER(ValueMlp), _vp, _i64, _vp]),
    "narde_value_rollout_league": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    "narde_turn_value_rollout_league": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _i64, _vp, _vp]),
    "narde_state_records": (_i32, [_i32, _i64, _vp, _vp, _vp, _vp, _u32, _vp, _vp]),
    "narde_value_playout": (_i32, [_vp, _i64, _vp, _i32, _i32, ctypes.POINTER(ValueMlp), ctypes.POINTER(ValueMlp), _u64,
                                   _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "narde_turn_value_playout": (_i32, [_vp, _i64, _vp, _i32, _i32, ctypes.POINTER(ValueMlp), ctypes.POINTER(ValueMlp),
                                        _u64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "narde_afterstates_records": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(ValueMlp), _i32, _vp, _vp,
                                         _vp]),
    "narde_turn_afterstates_records": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(ValueMlp), _i32, _vp,
                                              _vp, _vp]),
    "narde_rows_topk": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "narde_playout_pick": (_i32, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_turn_playout_pick": (_i32, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_records_lookahead": (_i32, [_vp, _i64, _vp, ctypes.POINTER(ValueMlp), _vp, _vp]),
    "narde_turn_records_lookahead": (_i32, [_vp, _i64, _vp, ctypes.POINTER(ValueMlp), _vp, _vp, _i64, _vp]),
    "narde_slot_pick": (_i32, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_turn_slot_pick": (_i32, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_value_td_trace": (_i32, [_vp, ctypes.POINTER(ValueMlpTrain), ctypes.c_float, _vp, _i64, _vp, _vp, _vp]),
    "narde_value_td_apply": (_i32, [_vp, ctypes.POINTER(ValueMlpTrain), _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                    ctypes.c_float, ctypes.c_float, _i32, _vp, _i64, _vp, _vp]),
    "narde_value_td_window": (_i32, [_vp, ctypes.POINTER(ValueMlpTrain), _i32, _vp, _vp, _vp, _vp, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_float, _vp, _i64, _vp, _vp]),
    "narde_value_fit": (_i32, [_i32, ctypes.POINTER(ValueMlpTrain), _i64, _vp, _vp, _vp, ctypes.c_float, _vp, _i64, _vp,
                               _vp, _vp]),
    "narde_playout_targets": (_i32, [_i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_value_td_window_grad": (_i32, [_vp, ctypes.POINTER(ValueMlpTrain), _i32, _vp, _vp, _vp, _vp, ctypes.c_float,
                                          ctypes.c_float, _vp, _i64, _vp, _vp, _vp]),
    "narde_value_fit_grad": (_i32, [_i32, ctypes.POINTER(ValueMlpTrain), _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                    _vp]),
    "narde_value_grad_norm": (_i32, [_i32, _i32, _vp, ctypes.c_float, _vp, _vp]),
    "narde_value_sgd_step": (_i32, [_i32, ctypes.POINTER(ValueMlpTrain), _vp, _vp, ctypes.c_float, _vp]),
    "narde_value_adam_step": (_i32, [_i32, ctypes.POINTER(ValueMlpTrain), _vp, _vp, _vp, _vp, _vp, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp]),
    "narde_policy_masked_argmax576": (_i32, [_i32, _vp, _i64, _vp, _i64, ctypes.c_float, _u64, _u32,
                                             _i32, _vp, _vp]),
    "narde_policy_masked_argmax576_dev": (_i32, [_i32, _vp, _i64, _vp, _i64, _vp, _u64, _vp, _i32, _vp,
                                                 _i64, _vp, _vp, _vp]),
    "narde_head_policy576_dev": (_i32, [_i32, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _u64, _vp, _i32,
                                        _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "narde_dqn_transition": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _i64, _vp]),
    "narde_per_sample": (_i32, [_i32, _vp, _vp, _i64, _i64, _u64, _vp, _vp, ctypes.c_double, _vp, _vp, _vp,
                                _vp, _vp]),
    "narde_per_prefix": (_i32, [_i32, _vp, _i64, ctypes.c_double, _vp, _vp, _vp, _i64, _vp]),
    "narde_gather_batch": (_i32, [_i32, _vp, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp]),
    "narde_rowmax_addend": (_i32, [_i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "narde_dqn_heads_forward": (_i32, [_i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp,
                                       _vp]),
    "narde_dqn_heads_backward": (_i32, [_i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp,
                                        _vp, _vp, _vp, _vp]),
    "narde_relu_bias_grad": (_i32, [_i32, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "narde_per_sample_gather": (_i32, [_i32, _vp, _vp, _i64, _i64, _u64, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i64,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_target_max2": (_i32, [_i32, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "narde_dqn_loss_prio": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_float, _vp, _vp, _vp,
                                   _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, ctypes.c_float, ctypes.c_float, _vp,
                                   _i64, _i64, _vp, _vp, _vp, ctypes.c_double, _vp]),
    "narde_adam_clip": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_float,
                               ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "narde_violates_block_rule": (_i32, [_i32, _vp, _i64, _vp, _vp]),
    "narde_host_legal_moves": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_host_step": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "narde_host_apply_moves": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "narde_host_violates_block_rule": (_i32, [_vp, _i64, _vp, _vp]),
}


class NardeLibraryError(RuntimeError):
    pass


class NardeValueError(NardeLibraryError, ValueError):
    """NARDE_EINVAL: an invalid argument or position."""


_lib = None


def load():
    """Load libnarde.so (raises NardeLibraryError if it is not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NardeLibraryError(
            f"libnarde.so not found at {LIB_PATH}: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != OK:
        msg = load().narde_last_error().decode(errors="replace")
        cls = NardeValueError if rc == -1 else NardeLibraryError
        raise cls(f"{what} failed ({rc}): {msg}")


def ptr(a):
    """Raw pointer of a numpy array / torch tensor / None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    return a.ctypes.data_as(ctypes.c_void_p)


class Handle:
    """Owns one narde_env (B envs resident on one device)."""

    def __init__(self, device, num_envs, env_id_offset=0, seed=0, dice_mode=DICE_ALL36,
                 max_episode_steps=1000):
        self.lib = load()
        h = ctypes.c_void_p()
        check(self.lib.narde_create(int(device), int(num_envs), int(env_id_offset),
                                    int(seed) & (2 ** 64 - 1), int(dice_mode),
                                    int(max_episode_steps), ctypes.byref(h)), "narde_create")
        self.h = h
        self.device = int(device)
        self.num_envs = int(num_envs)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.narde_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, *args):
        check(getattr(self.lib, name)(self.h, *args), name)

    @property
    def ply(self):
        t = _u32()
        check(self.lib.narde_get_ply(self.h, ctypes.byref(t)), "narde_get_ply")
        return t.value

    @ply.setter
    def ply(self, t):
        check(self.lib.narde_set_ply(self.h, int(t) & 0xFFFFFFFF), "narde_set_ply")


_host_handle = None


def host_handle():
    """Process-wide handle used by the scalar facade for its host calls."""
    global _host_handle
    if _host_handle is None:
        dev = int(os.environ.get("NARDE_DEVICE", "0"))
        _host_handle = Handle(dev, 1)
    return _host_handle
