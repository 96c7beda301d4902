// narde.hip -- HIP kernels (gfx950) + the C ABI of libnarde (include/narde.h).
//
// One lane = one env.  Each env is a 32-byte record split into two planar
// 16-byte planes (narde_rules.h), so every wave-wide load/store of state is
// a single contiguous 1 KiB transaction.  The rules engine (narde_rules.h) is
// branch-light bitmask arithmetic on 24-bit point masks held in VGPRs.
//
// One translation unit; the device code is split by role into headers
// included below, in order:
//   device_common.h     build knobs, env planes, the device RNG draws
//   kernels_state.h     reset, set/get state, peek dice, get_valid_moves
//                       (k_legal), apply, statistics, block rule
//   kernels_full4.h     k_legal_full, with full4_wave.h: the
//                       wave-cooperative FULL4 turn
//   kernels_rollout.h   the timed path: per-ply outputs, k_step (API step),
//                       the producer/consumer rollouts k_rollout_pc (REF2)
//                       and k_rollout_pp_full (FULL4)
//   kernels_agent.h     observations, move masks, the policy kernel, the DQN
//                       transition
//   kernels_rows.h      afterstate rows, what both rule sets share: the wave
//                       helpers, the row stores, the scored rows (a value
//                       MLP in the fill pass), k_aft_scan, k_aft_pick
//   kernels_afterstates.h  REF2 afterstates: the play enumeration
//                       (k_aft_count, k_aft_fill, k_aft_fill_scored)
//   kernels_lookahead.h  REF2 two-ply lookahead: the record fill and the
//                       expected-best-reply pass (k_aft_fill_rec, k_aft_look)
//   kernels_value_rollout.h  REF2 value-greedy games in one launch, a net per
//                       colour (k_value_rollout)
//   kernels_turn_afterstates.h  FULL4 whole-turn afterstates: the level walk
//                       (k_turn_count, k_turn_fill, k_turn_overflow, and the
//                       scored fills)
//   kernels_turn_lookahead.h  FULL4 two-ply lookahead: the record fills, the
//                       reply walk per (row, roll), its overflow pass and the
//                       mean (k_turn_fill_rec, k_turn_look, k_turn_look_overflow,
//                       k_turn_look_mean); the look passes of both rule sets
//                       have a second instantiation over a caller's records
//                       (behind k_turn_look_pack here)
//   kernels_turn_value_rollout.h  FULL4 value-greedy games in one launch: the
//                       picking consumer of the level walk inside a ply loop
//                       (k_turn_value_rollout)
//   kernels_value_playout.h  Monte-Carlo playouts of given positions under
//                       value nets, REF2: the rollout's ply from a caller's
//                       records to the end of the game (k_state_records,
//                       k_playout_zero, k_value_playout)
//   kernels_turn_value_playout.h  the same over FULL4 whole turns
//                       (k_turn_value_playout)
//   kernels_playout_pick.h  playout-greedy play: the scored fills with the
//                       rows' records as an output, an env's top-K rows as
//                       playout roots, the pick over the playouts' sums
//                       (k_aft_fill_records, k_turn_fill_records,
//                       k_rows_topk, k_playout_pick), the pick over given
//                       slot scores (k_slot_pick)
//   kernels_td.h        TD(lambda) on the value MLP: the trace pass, the TD
//                       errors, the slab sums and the weight update
//   kernels_td_window.h  windowed TD(lambda): the window's values, returns and
//                       slab gradient sums (k_tdw_values, k_tdw_returns,
//                       k_tdw_grad)
//   kernels_value_fit.h  the supervised fit of given records to given float
//                       targets, and the playout targets (k_fit_grad,
//                       k_fit_loss, k_playout_targets)
//   kernels_league.h    the two value rollouts with a net per env and colour
//                       from a table (k_net_table_write,
//                       k_value_rollout_league, k_turn_value_rollout_league)
// This file keeps the handle, the host-side checks and every C entry point.
// The DQN learner kernels are a second translation unit (dqn_learner.hip);
// host_common.h: the host helpers the two share.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <initializer_list>
#include <new>
#include <type_traits>

#include "../../include/narde.h"
#include "host_common.h"
#include "narde_rules.h"

using namespace narde;
using namespace narde_host;

thread_local char narde_host::g_err[512] = "";

#include "device_common.h"
#include "kernels_state.h"
#include "kernels_full4.h"
#include "kernels_rollout.h"
#include "kernels_agent.h"
#include "kernels_rows.h"
#include "kernels_afterstates.h"
#include "kernels_lookahead.h"
#include "kernels_value_rollout.h"
#include "kernels_turn_afterstates.h"
#include "kernels_turn_lookahead.h"
#include "kernels_turn_value_rollout.h"
#include "kernels_value_playout.h"
#include "kernels_turn_value_playout.h"
#include "kernels_playout_pick.h"
#include "kernels_td.h"
#include "kernels_td_window.h"
#include "kernels_value_fit.h"
#include "kernels_value_optim.h"
#include "kernels_league.h"

namespace {

inline int grid(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

// The narde_host_* calls: at most kHostCap envs, each array in a slot of its
// own in the handle's staging buffers (Stage, below, which checks this size):
// the most bytes per env one direction of one call stages (narde_host_step's
// seven outputs) and each array's rounding to a slot.
constexpr int64_t kHostCap = 4096;
constexpr size_t kStageSlot = 256;
constexpr size_t kStageEnvBytes = 130;
constexpr size_t kStageArrays = 7;
constexpr size_t kStageBytes = kHostCap * kStageEnvBytes + kStageArrays * kStageSlot;

constexpr size_t stage_slot(size_t bytes) { return (bytes + kStageSlot - 1) & ~(kStageSlot - 1); }

}  // namespace

// ---------------------------------------------------------------- handle
struct narde_env {
  int device;
  int64_t n;
  int64_t env0;
  uint64_t seed;
  int dice_mode;
  int max_steps;
  uint32_t epoch;
  Planes pl;
  // host-call staging (scalar facade)
  Planes hpl;
  uint8_t* h_in;   // pinned
  uint8_t* h_out;  // pinned
  uint8_t* d_in;
  uint8_t* d_out;
  hipStream_t hstream;
  // narde_turn_afterstates' workspace, made on its first call: the overflow
  // list [1 + n] and the overflow launches' frontier slab
  int32_t* turn_ovf;
  uint8_t* turn_slab;
};

namespace {

Rng rng_of(const narde_env* e) {
  Rng g;
  g.env0 = (uint32_t)e->env0;
  g.k0 = (uint32_t)e->seed;
  g.k1 = (uint32_t)(e->seed >> 32);
  g.dice_mode = e->dice_mode;
  return g;
}

// k_step's arguments: n envs of planes pl (the handle's own or its host
// envs), REF2 codes `actions` or a FULL4 `play`
StepArgs step_args(const narde_env* e, const Planes& pl, int64_t n, int max_steps, int autoreset,
                   const int16_t* actions, const int8_t* play, const uint8_t* dice, const Outs& out) {
  return StepArgs{pl, (int)n, rng_of(e), max_steps, autoreset, actions, play, dice, out};
}

// One rollout launch: the kernel -- REF2's k_rollout_pc or FULL4's
// producer/consumer pairs k_rollout_pp_full, in the
// instantiation with per-ply outputs only when one is asked for -- its
// geometry and its six arguments.  `last` is the output one rule set alone
// has: REF2's codes used (int16_t[.][n][2]), FULL4's sub-moves (uint64_t[.][n]).
struct RolloutLaunch {
  const void* kernel;
  const char* name;  // in a failed launch's error text
  dim3 grid, block;
  Planes pl;
  int n;
  Rng g;  // seed, env ids, dice law (the ply counter is each env's record word)
  int plies;
  int max_steps;
  Outs out;
  // hipLaunchKernel's argument array; valid while *this stays where it is
  void bind(void* (&args)[6]) {
    args[0] = &pl, args[1] = &n, args[2] = &g, args[3] = &plies, args[4] = &max_steps, args[5] = &out;
  }
  int launch(hipStream_t stream) {
    void* args[6];
    bind(args);
    (void)hipLaunchKernel(kernel, grid, block, args, 0, stream);
    return check_launch(name);
  }
};

RolloutLaunch rollout_launch(const narde_env* e, int full, int plies, int32_t* obs, int32_t* reward,
                             uint8_t* terminated, uint8_t* truncated, uint64_t* legal, void* last, int64_t* totals) {
  const bool any = obs || reward || terminated || truncated || legal || last;
  return RolloutLaunch{full ? (any ? (const void*)k_rollout_pp_full<true> : (const void*)k_rollout_pp_full<false>)
                            : (any ? (const void*)k_rollout_pc<true> : (const void*)k_rollout_pc<false>),
                       full ? "k_rollout_pp_full" : "k_rollout", dim3((unsigned)((e->n + kPcEnvs - 1) / kPcEnvs)),
                       dim3(kPcThreads), e->pl, (int)e->n, rng_of(e), plies, e->max_steps,
                       Outs{obs, reward, terminated, truncated, legal, full ? nullptr : (int16_t*)last,
                            full ? (uint64_t*)last : nullptr, totals}};
}

bool valid_position(const int8_t* board, const uint8_t* off, const uint8_t* ft, const int8_t* player,
                    int64_t i) {
  int w = 0, b = 0;
  for (int p = 0; p < 24; ++p) {
    const int v = board[i * 24 + p];
    if (v > 15 || v < -15) return false;
    if (v > 0) w += v; else b -= v;
  }
  if (off[2 * i] > 15 || off[2 * i + 1] > 15) return false;
  if (w + off[2 * i] > 15 || b + off[2 * i + 1] > 15) return false;
  if (player && player[i] != 1 && player[i] != -1) return false;
  (void)ft;
  return true;
}

// The two afterstate expansions' (narde_afterstates, narde_turn_afterstates)
// argument checks.  max_rows: the kind's rows-per-env bound; column: its
// action column, `align`-byte words; misaligned: the alignment error's text.
int check_expand(const narde_env* e, int64_t cap, const int32_t* offsets, int max_rows, const float* feat,
                 const int32_t* obs, const void* column, unsigned align, const char* misaligned) {
  if (!e || !offsets) return fail(NARDE_EINVAL, "NULL argument");
  if (cap < 0) return fail(NARDE_EINVAL, "cap %lld is negative", (long long)cap);
  if (e->n * (int64_t)max_rows >= (int64_t(1) << 31))
    return fail(NARDE_EINVAL, "too many envs for 32-bit row offsets (B x %d must stay below 2^31)", max_rows);
  if (!aligned16(feat) || !aligned16(obs) || (reinterpret_cast<uintptr_t>(column) % align))
    return fail(NARDE_EINVAL, "%s", misaligned);
  return NARDE_OK;
}

// The scored expansions' (narde_afterstates_scored,
// narde_turn_afterstates_scored) checks of the net, and the kernels' view of it.
int check_value_net(const narde_value_mlp* net, int perspective, float* value, ValNet& vn) {
  if (!net || !value) return fail(NARDE_EINVAL, "NULL argument");
  return check_value_mlp(net, perspective, value, kValLdMax, vn);
}

// narde_value_td_trace's and narde_value_td_apply's checks of the net and the
// trace rows, and the kernels' view of the net
static_assert(kTdSlab == NARDE_TD_SLAB, "narde.h and narde_rules.h state the same slab");
int check_td(const narde_env* e, const narde_value_mlp_train* net, const float* trace, int64_t ld_trace,
             const float* v, const uint8_t* black, TdNet& tn) {
  if (!e || !net || !trace || !v || !black) return fail(NARDE_EINVAL, "NULL argument");
  if (const int rc = check_mlp_fields(net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->hidden, net->hidden_act,
                                      net->out_act, kValLdMax))
    return rc;
  if (net->w1 && net->ld_w1 < 198) return fail(NARDE_EINVAL, "ld_w1 %lld below 198", (long long)net->ld_w1);
  const int64_t P = td_row_floats(net->hidden);
  if (ld_trace < P || (ld_trace & 3))
    return fail(NARDE_EINVAL, "ld_trace %lld: a multiple of 4, at least 200 x hidden + 1 = %lld", (long long)ld_trace,
                (long long)P);
  if (!aligned16(trace)) return fail(NARDE_EINVAL, "trace must be 16-B aligned");
  tn = TdNet{net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->w1, net->ld_w1, net->hidden, net->hidden_act,
             net->out_act};
  return NARDE_OK;
}

// REF2's expansion: the count pass, the scan, and the fill -- with the
// rows' values (vn) the scored one, with the rows' public records (pub) the
// records fills of narde_afterstates_records
int expand_plays(narde_env* e, const AftArgs& a, const ValNet* vn, hipStream_t st, const AftRec* pub = nullptr) {
  const int cw = kAftCountBlock / 64, fw = kAftFillBlock / 64;
  k_aft_count<<<(unsigned)((e->n + cw - 1) / cw), kAftCountBlock, 0, st>>>(a);
  if (const int rc = check_launch("k_aft_count")) return rc;
  k_aft_scan<<<1, kAftScanBlock, 0, st>>>(a.offsets, (int)e->n);
  if (const int rc = check_launch("k_aft_scan")) return rc;
  if (a.cap == 0 || !(a.row_env || a.codes || a.feat || a.obs || a.reward || vn || pub)) return NARDE_OK;
  if (pub) {
    if (vn)
      k_aft_fill_scored_records<<<(unsigned)((e->n + fw - 1) / fw), kAftFillBlock, 0, st>>>(a, *vn, *pub);
    else
      k_aft_fill_records<<<(unsigned)((e->n + fw - 1) / fw), kAftFillBlock, 0, st>>>(a, *pub);
    return check_launch("k_aft_fill_records");
  }
  if (vn) {
    k_aft_fill_scored<<<(unsigned)((e->n + fw - 1) / fw), kAftFillBlock, 0, st>>>(a, *vn);
    return check_launch("k_aft_fill_scored");
  }
  k_aft_fill<<<(unsigned)((e->n + fw - 1) / fw), kAftFillBlock, 0, st>>>(a);
  return check_launch("k_aft_fill");
}

// The handle's FULL4 workspace, made by the first call that needs it (the
// expansions below; narde_turn_records_lookahead, for the slab)
int turn_workspace(narde_env* e, hipStream_t st) {
  if (!e->turn_slab) {
    // the workspace belongs to the handle and is made once, outside capture
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
      return fail(NARDE_EINVAL, "the first narde_turn_afterstates call of a handle allocates its workspace: "
                                "make it outside stream capture");
    hipError_t err = hipMalloc(&e->turn_ovf, (size_t)(e->n + 1) * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc(&e->turn_slab, (size_t)kTurnOvfWaves * kTurnSlabWave);
    if (err != hipSuccess) {
      (void)hipFree(e->turn_ovf);
      (void)hipFree(e->turn_slab);
      e->turn_ovf = nullptr;
      e->turn_slab = nullptr;
      return fail(NARDE_ENOMEM, "turn afterstate workspace: %s", hipGetErrorString(err));
    }
  }
  return NARDE_OK;
}

// FULL4's: the handle's workspace on its first call, the count passes, the
// scan, the fills (scored with vn; with tr the record fills of the lookahead,
// whose own passes the caller launches behind them; with pub the records fills
// of narde_turn_afterstates_records, scored if vn is given)
int expand_turns(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* row_env, int8_t* play,
                 float* feat, int32_t* obs, int8_t* reward, const ValNet* vn, hipStream_t st,
                 const TurnRec* tr = nullptr, const TurnRec* pub = nullptr) {
  if (const int rc = turn_workspace(e, st)) return rc;
  TurnArgs a{e->pl, (int)e->n, rng_of(e), dice, cap, offsets, row_env, play, feat, obs, reward, e->turn_ovf,
             e->turn_slab};
  const int cw = kTurnCountBlock / 64, fw = kTurnFillBlock / 64;
  HIP_TRY(hipMemsetAsync(e->turn_ovf, 0, sizeof(int32_t), st));
  k_turn_count<<<(unsigned)((e->n + cw - 1) / cw), kTurnCountBlock, 0, st>>>(a);
  if (const int rc = check_launch("k_turn_count")) return rc;
  k_turn_overflow<false><<<kTurnOvfWaves, 64, 0, st>>>(a);
  if (const int rc = check_launch("k_turn_overflow<count>")) return rc;
  k_aft_scan<<<1, kAftScanBlock, 0, st>>>(offsets, (int)e->n);
  if (const int rc = check_launch("k_aft_scan")) return rc;
  if (cap == 0 || !(row_env || play || feat || obs || reward || vn || tr || pub)) return NARDE_OK;
  if (pub) {
    const unsigned g = (unsigned)((e->n + fw - 1) / fw);
    if (vn) {
      k_turn_fill_records<true><<<g, kTurnFillBlock, 0, st>>>(a, *vn, *pub);
      if (const int rc = check_launch("k_turn_fill_records")) return rc;
      k_turn_overflow_records<true><<<kTurnOvfWaves, 64, 0, st>>>(a, *vn, *pub);
    } else {
      k_turn_fill_records<false><<<g, kTurnFillBlock, 0, st>>>(a, ValNet{}, *pub);
      if (const int rc = check_launch("k_turn_fill_records")) return rc;
      k_turn_overflow_records<false><<<kTurnOvfWaves, 64, 0, st>>>(a, ValNet{}, *pub);
    }
    return check_launch("k_turn_overflow_records");
  }
  if (tr) {
    k_turn_fill_rec<<<(unsigned)((e->n + fw - 1) / fw), kTurnFillBlock, 0, st>>>(a, *tr);
    if (const int rc = check_launch("k_turn_fill_rec")) return rc;
    k_turn_overflow_rec<<<kTurnOvfWaves, 64, 0, st>>>(a, *tr);
    return check_launch("k_turn_overflow_rec");
  }
  if (vn) {
    k_turn_fill_scored<<<(unsigned)((e->n + fw - 1) / fw), kTurnFillBlock, 0, st>>>(a, *vn);
    if (const int rc = check_launch("k_turn_fill_scored")) return rc;
    k_turn_overflow_scored<<<kTurnOvfWaves, 64, 0, st>>>(a, *vn);
    return check_launch("k_turn_overflow_scored");
  }
  k_turn_fill<<<(unsigned)((e->n + fw - 1) / fw), kTurnFillBlock, 0, st>>>(a);
  if (const int rc = check_launch("k_turn_fill")) return rc;
  k_turn_overflow<true><<<kTurnOvfWaves, 64, 0, st>>>(a);
  return check_launch("k_turn_overflow<fill>");
}

// The two picks (narde_afterstate_pick, narde_turn_pick): the checks and the
// launch of k_aft_pick over the kind's action column of words W (kNoRow for
// an env with no row).  kernel, misaligned: the kind's error texts.
template <typename W, int kNoRow>
int pick_rows(narde_env* e, const int32_t* offsets, const void* column, int64_t cap, const float* value,
              int64_t ld_value, int perspective, const float* epsilon, uint64_t seed, const int64_t* tag, void* out,
              int32_t* row, void* stream, const char* kernel, const char* misaligned) {
  if (!e || !offsets || !column || !value || !out) return fail(NARDE_EINVAL, "NULL argument");
  if (cap < 0) return fail(NARDE_EINVAL, "cap %lld is negative", (long long)cap);
  if (perspective != 0 && perspective != 1)
    return fail(NARDE_EINVAL, "perspective must be 0 (the mover's values) or 1 (white's)");
  if (ld_value < 1) return fail(NARDE_EINVAL, "bad value stride");
  if (epsilon && !tag) return fail(NARDE_EINVAL, "exploration needs a tag");
  if ((reinterpret_cast<uintptr_t>(column) % sizeof(W)) || (reinterpret_cast<uintptr_t>(out) % sizeof(W)))
    return fail(NARDE_EINVAL, "%s", misaligned);
  DeviceGuard dg(e->device);
  k_aft_pick<W, kNoRow><<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(
      e->pl, (int)e->n, offsets, static_cast<const W*>(column), cap, value, ld_value, perspective, epsilon, tag,
      (uint32_t)seed, (uint32_t)(seed >> 32), static_cast<W*>(out), row);
  return check_launch(kernel);
}

// narde_afterstates_records' and narde_turn_afterstates_records' checks behind
// check_expand's: the records, and the net with its values or neither
int check_records(const void* records, const narde_value_mlp* net, int perspective, float* value, ValNet& vn) {
  if (!records) return fail(NARDE_EINVAL, "NULL records (without them the call is the scored expansion)");
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  if ((net != nullptr) != (value != nullptr))
    return fail(NARDE_EINVAL, "net and value must both be set or both be NULL");
  if (net) return check_value_net(net, perspective, value, vn);
  return NARDE_OK;
}

// narde_playout_pick's and narde_turn_playout_pick's checks and launch, as
// pick_rows: words W of the kind's action column, kNoRow for no candidate
template <typename W, int kNoRow>
int playout_pick_rows(narde_env* e, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld_value,
                      const int8_t* reward, const void* column, int trials, const int32_t* sums, const float* leaf,
                      void* out, int32_t* row, float* score, void* stream, const char* misaligned) {
  if (!e || !sel || !value || !reward || !sums || !column || !out) return fail(NARDE_EINVAL, "NULL argument");
  if (k < 1 || k > NARDE_TOPK_MAX) return fail(NARDE_EINVAL, "k %d outside 1 .. NARDE_TOPK_MAX = %d", k, NARDE_TOPK_MAX);
  if (trials < 1) return fail(NARDE_EINVAL, "trials %d must be at least 1", trials);
  if (cap < 0) return fail(NARDE_EINVAL, "cap %lld is negative", (long long)cap);
  if (ld_value < 1) return fail(NARDE_EINVAL, "bad value stride");
  if (e->n * (int64_t)k * (int64_t)trials >= (int64_t(1) << 31))
    return fail(NARDE_EINVAL, "B x k x trials must stay below 2^31 (k %d, trials %d)", k, trials);
  if ((reinterpret_cast<uintptr_t>(column) % sizeof(W)) || (reinterpret_cast<uintptr_t>(out) % sizeof(W)))
    return fail(NARDE_EINVAL, "%s", misaligned);
  DeviceGuard dg(e->device);
  const PlayoutPickArgs a{e->pl, (int)e->n, k, trials, sel, cap, value, ld_value, reward, sums, leaf, row, score};
  k_playout_pick<W, kNoRow><<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(a, static_cast<const W*>(column),
                                                                            static_cast<W*>(out));
  return check_launch("k_playout_pick");
}

// narde_slot_pick's and narde_turn_slot_pick's: the same with the caller's
// slot scores in place of the trials and sums
template <typename W, int kNoRow>
int slot_pick_rows(narde_env* e, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld_value,
                   const int8_t* reward, const void* column, const float* slot_score, void* out, int32_t* row,
                   float* score, void* stream, const char* misaligned) {
  if (!e || !sel || !value || !reward || !slot_score || !column || !out) return fail(NARDE_EINVAL, "NULL argument");
  if (k < 1 || k > NARDE_TOPK_MAX) return fail(NARDE_EINVAL, "k %d outside 1 .. NARDE_TOPK_MAX = %d", k, NARDE_TOPK_MAX);
  if (cap < 0) return fail(NARDE_EINVAL, "cap %lld is negative", (long long)cap);
  if (ld_value < 1) return fail(NARDE_EINVAL, "bad value stride");
  if (e->n * (int64_t)k >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "B x k must stay below 2^31 (k %d)", k);
  if ((reinterpret_cast<uintptr_t>(column) % sizeof(W)) || (reinterpret_cast<uintptr_t>(out) % sizeof(W)))
    return fail(NARDE_EINVAL, "%s", misaligned);
  DeviceGuard dg(e->device);
  const SlotPickArgs a{e->pl, (int)e->n, k, sel, cap, value, ld_value, reward, slot_score, row, score};
  k_slot_pick<W, kNoRow><<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(a, static_cast<const W*>(column),
                                                                         static_cast<W*>(out));
  return check_launch("k_slot_pick");
}

// narde_records_lookahead's and narde_turn_records_lookahead's checks of the
// handle, the records, the net and the values, and the kernels' view of the net
int check_records_lookahead(const narde_env* e, int64_t n, const void* records, const narde_value_mlp* net,
                            float* value, ValNet& vn) {
  if (!e || !net || !value) return fail(NARDE_EINVAL, "NULL argument");
  if (const int rc = check_given_records(n, records)) return rc;
  return check_value_net(net, 1, value, vn);
}

// a value or league rollout kernel's launch, `waves` one-wave workgroups: its
// <true> instantiation if the call has a records column, else its <false> one
template <class... P, class... A>
int launch_rollout(bool records, void (*with)(P...), void (*without)(P...), int64_t waves, void* stream,
                   const char* what, const A&... args) {
  (records ? with : without)<<<(unsigned)waves, 64, 0, (hipStream_t)stream>>>(args...);
  return check_launch(what);
}

}  // namespace

extern "C" {

int narde_version(void) { return 2; }
const char* narde_last_error(void) { return g_err; }

int narde_create(int device, int64_t num_envs, int64_t env_id_offset, uint64_t seed, int dice_mode,
                 int max_episode_steps, narde_env** out) {
  if (!out) return fail(NARDE_EINVAL, "out is NULL");
  *out = nullptr;
  if (num_envs <= 0 || num_envs > (int64_t(1) << 31) - kBlock)
    return fail(NARDE_EINVAL, "num_envs %lld out of range", (long long)num_envs);
  if (env_id_offset < 0 || env_id_offset + num_envs > (int64_t(1) << 32))
    return fail(NARDE_EINVAL, "global env ids must fit in 32 bits");
  if (dice_mode != NARDE_DICE_ALL36 && dice_mode != NARDE_DICE_NODOUBLES)
    return fail(NARDE_EINVAL, "bad dice_mode %d", dice_mode);
  if (max_episode_steps < 0 || max_episode_steps > 65535)
    return fail(NARDE_EINVAL, "max_episode_steps must be in [0, 65535]");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(NARDE_EINVAL, "device %d of %d", device, ndev);
  DeviceGuard dg(device);
  narde_env* e = new (std::nothrow) narde_env();
  if (!e) return fail(NARDE_ENOMEM, "host alloc");
  e->device = device;
  e->n = num_envs;
  e->env0 = env_id_offset;
  e->seed = seed;
  e->dice_mode = dice_mode;
  e->max_steps = max_episode_steps;
  hipError_t err = hipSuccess;
  err = hipMalloc(&e->pl.p0, num_envs * sizeof(uint4));
  if (err == hipSuccess) err = hipMalloc(&e->pl.p1, num_envs * sizeof(uint4));
  if (err == hipSuccess) err = hipMalloc(&e->pl.stats, num_envs * sizeof(int4));
  if (err == hipSuccess) err = hipMalloc(&e->hpl.p0, kHostCap * sizeof(uint4));
  if (err == hipSuccess) err = hipMalloc(&e->hpl.p1, kHostCap * sizeof(uint4));
  if (err == hipSuccess) err = hipMalloc(&e->hpl.stats, kHostCap * sizeof(int4));
  if (err == hipSuccess) err = hipMalloc(&e->d_in, kStageBytes);
  if (err == hipSuccess) err = hipMalloc(&e->d_out, kStageBytes);
  if (err == hipSuccess) err = hipHostMalloc(&e->h_in, kStageBytes, hipHostMallocDefault);
  if (err == hipSuccess) err = hipHostMalloc(&e->h_out, kStageBytes, hipHostMallocDefault);
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&e->hstream, hipStreamNonBlocking);
  if (err != hipSuccess) {
    narde_destroy(e);
    return fail(NARDE_ENOMEM, "device alloc for %lld envs: %s", (long long)num_envs,
                hipGetErrorString(err));
  }
  k_reset<<<grid(num_envs), kBlock, 0, e->hstream>>>(e->pl, (int)num_envs, rng_of(e), 0u, nullptr,
                                                     (int64_t)0, nullptr, 0);
  int rc = check_launch("k_reset");
  if (rc == NARDE_OK) {
    err = hipStreamSynchronize(e->hstream);
    if (err != hipSuccess) rc = fail(NARDE_EHIP, "reset sync: %s", hipGetErrorString(err));
  }
  if (rc != NARDE_OK) {
    narde_destroy(e);
    return rc;
  }
  e->epoch = 1;
  *out = e;
  return NARDE_OK;
}

int narde_destroy(narde_env* e) {
  if (!e) return NARDE_OK;
  DeviceGuard dg(e->device);
  if (e->hstream) (void)hipStreamSynchronize(e->hstream);
  (void)hipFree(e->pl.p0); (void)hipFree(e->pl.p1); (void)hipFree(e->pl.stats);
  (void)hipFree(e->hpl.p0); (void)hipFree(e->hpl.p1); (void)hipFree(e->hpl.stats);
  (void)hipFree(e->d_in); (void)hipFree(e->d_out);
  (void)hipFree(e->turn_ovf); (void)hipFree(e->turn_slab);
  if (e->h_in) (void)hipHostFree(e->h_in);
  if (e->h_out) (void)hipHostFree(e->h_out);
  if (e->hstream) (void)hipStreamDestroy(e->hstream);
  delete e;
  return NARDE_OK;
}

int64_t narde_num_envs(const narde_env* e) { return e ? e->n : -1; }

int narde_get_ply(const narde_env* e, uint32_t* t) {
  if (!e || !t) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(t, reinterpret_cast<const char*>(e->pl.p1) + 12, sizeof(uint32_t),
                    hipMemcpyDeviceToHost));
  return NARDE_OK;
}

int narde_set_ply(narde_env* e, uint32_t t) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  DeviceGuard dg(e->device);
  // every step / rollout still queued on any stream of the device first (they
  // advance t): the private stream alone is not ordered with the caller's
  HIP_TRY(hipDeviceSynchronize());
  k_set_ply<<<grid(e->n), kBlock, 0, e->hstream>>>(e->pl, (int)e->n, t);
  int rc = check_launch("k_set_ply");
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->hstream));
  return NARDE_OK;
}

int narde_reset(narde_env* e, const uint8_t* mask, const uint8_t* opening, int pairs, void* stream) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  if (opening && pairs <= 0) return fail(NARDE_EINVAL, "opening draws need pairs >= 1");
  DeviceGuard dg(e->device);
  k_reset<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), e->epoch, mask,
                                                           (int64_t)-1, opening, opening ? pairs : 0);
  e->epoch += 1;
  return check_launch("k_reset");
}

int narde_set_state(narde_env* e, const int8_t* board, const uint8_t* off, const uint8_t* ft,
                    const int8_t* player, const uint16_t* elapsed, void* stream) {
  if (!e || !board || !off || !ft || !player) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_set_state<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, board, off, ft, player,
                                                              elapsed, 1);
  return check_launch("k_set_state");
}

int narde_get_state(narde_env* e, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player,
                    uint16_t* elapsed, void* stream) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  DeviceGuard dg(e->device);
  k_get_state<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, board, off, ft, player,
                                                              elapsed);
  return check_launch("k_get_state");
}

int narde_peek_dice(narde_env* e, uint8_t* dice, void* stream) {
  if (!e || !dice) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_peek_dice<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), dice);
  return check_launch("k_peek_dice");
}

int narde_legal_moves(narde_env* e, const uint8_t* dice, int16_t* out_count, int8_t* out_moves,
                      uint64_t* out_compact, void* stream) {
  if (!e || !out_count) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_legal<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), dice,
                                                          out_count, out_moves, out_compact);
  return check_launch("k_legal");
}

int narde_step(narde_env* e, const int16_t* actions, const uint8_t* dice, int32_t* obs,
               int32_t* reward, uint8_t* terminated, uint8_t* truncated, uint64_t* legal_compact,
               int16_t* actions_out, int autoreset, void* stream) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  DeviceGuard dg(e->device);
  k_step<false><<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(
      step_args(e, e->pl, e->n, e->max_steps, autoreset, actions, nullptr, dice,
                Outs{obs, reward, terminated, truncated, legal_compact, actions_out, nullptr}));
  return check_launch("k_step");
}

int narde_step_full(narde_env* e, const int8_t* play, const uint8_t* dice, int32_t* obs, int32_t* reward,
                    uint8_t* terminated, uint8_t* truncated, uint64_t* legal_first, uint64_t* played,
                    int autoreset, void* stream) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  DeviceGuard dg(e->device);
  k_step<true><<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(
      step_args(e, e->pl, e->n, e->max_steps, autoreset, nullptr, play, dice,
                Outs{obs, reward, terminated, truncated, legal_first, nullptr, played}));
  return check_launch("k_step<full>");
}

// The rollout launches.  narde_rollout_timed brackets them with two
// hipEventRecord markers: hipExtLaunchKernel's packet-level start / stop
// events were measured too and cost ~12 us more per host round trip of one
// launch than the markers' ~4 us (tools/diag/single_launch.py, one box).
int narde_rollout_timed(narde_env* e, int full, int plies, int32_t* obs, int32_t* reward, uint8_t* terminated,
                        uint8_t* truncated, uint64_t* legal, void* last, void* ev_start, void* ev_stop,
                        int64_t* totals, void* stream) {
  if (!e || plies < 0) return fail(NARDE_EINVAL, "bad argument");
  if (totals && plies == 0) return fail(NARDE_EINVAL, "totals rows need a launch (plies > 0)");
  DeviceGuard dg(e->device);
  RolloutLaunch l = rollout_launch(e, full, plies, obs, reward, terminated, truncated, legal, last, totals);
  if (ev_start && hipEventRecord((hipEvent_t)ev_start, (hipStream_t)stream) != hipSuccess)
    return fail(NARDE_EHIP, "hipEventRecord(ev_start) failed");
  if (plies > 0)
    if (const int rc = l.launch((hipStream_t)stream)) return rc;
  if (ev_stop && hipEventRecord((hipEvent_t)ev_stop, (hipStream_t)stream) != hipSuccess)
    return fail(NARDE_EHIP, "hipEventRecord(ev_stop) failed");
  return NARDE_OK;
}

int narde_rollout(narde_env* e, int plies, int32_t* obs, int32_t* reward, uint8_t* terminated,
                  uint8_t* truncated, uint64_t* legal_compact, int16_t* actions_out, void* stream) {
  if (e && plies == 0) return NARDE_OK;
  return narde_rollout_timed(e, 0, plies, obs, reward, terminated, truncated, legal_compact, actions_out, nullptr,
                             nullptr, nullptr, stream);
}

int narde_selfplay(narde_env* e, int plies, void* stream) {
  return narde_rollout(e, plies, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int narde_rollout_full(narde_env* e, int plies, int32_t* obs, int32_t* reward, uint8_t* terminated,
                       uint8_t* truncated, uint64_t* legal_first, uint64_t* played, void* stream) {
  if (e && plies == 0) return NARDE_OK;
  return narde_rollout_timed(e, 1, plies, obs, reward, terminated, truncated, legal_first, played, nullptr, nullptr,
                             nullptr, stream);
}

int narde_selfplay_full(narde_env* e, int plies, void* stream) {
  return narde_rollout_full(e, plies, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

// narde_rollout_timed pre-bound (round 6): everything but the launch is done
// once at create -- argument checks, the device check, the kernel chosen,
// its arguments packed -- so the timed call is one ctypes argument and
// three runtime calls (event, hipLaunchKernel, event), no device switch.
struct narde_rollout_plan {
  RolloutLaunch l;
  void* args[6];
  hipEvent_t ev0, ev1;
  hipStream_t stream;
};

int narde_rollout_plan_create(narde_env* e, int full, int plies, int32_t* obs, int32_t* reward, uint8_t* terminated,
                              uint8_t* truncated, uint64_t* legal, void* last, void* ev_start, void* ev_stop,
                              int64_t* totals, void* stream, void** plan) {
  if (!e || !plan || plies <= 0) return fail(NARDE_EINVAL, "bad argument (a plan needs plies > 0)");
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != e->device)
    return fail(NARDE_EINVAL, "the calling thread's current device must be the env's");
  narde_rollout_plan* p = new (std::nothrow) narde_rollout_plan();
  if (!p) return fail(NARDE_ENOMEM, "out of host memory");
  p->l = rollout_launch(e, full, plies, obs, reward, terminated, truncated, legal, last, totals);
  p->l.bind(p->args);
  p->ev0 = (hipEvent_t)ev_start;
  p->ev1 = (hipEvent_t)ev_stop;
  p->stream = (hipStream_t)stream;
  *plan = p;
  return NARDE_OK;
}

int narde_rollout_plan_launch(void* plan) {
  narde_rollout_plan* p = (narde_rollout_plan*)plan;
  if (!p) return fail(NARDE_EINVAL, "NULL plan");
  if (p->ev0 && hipEventRecord(p->ev0, p->stream) != hipSuccess) return fail(NARDE_EHIP, "hipEventRecord(ev_start) failed");
  if (hipLaunchKernel(p->l.kernel, p->l.grid, p->l.block, p->args, 0, p->stream) != hipSuccess)
    return fail(NARDE_EHIP, "hipLaunchKernel(k_rollout) failed");
  if (p->ev1 && hipEventRecord(p->ev1, p->stream) != hipSuccess) return fail(NARDE_EHIP, "hipEventRecord(ev_stop) failed");
  return NARDE_OK;
}

int narde_rollout_plan_destroy(void* plan) {
  delete (narde_rollout_plan*)plan;
  return NARDE_OK;
}

int narde_timing_event_create(int device, unsigned flags, void** event) {
  if (!event) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(device);
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, flags) != hipSuccess) return fail(NARDE_EHIP, "hipEventCreateWithFlags failed");
  *event = ev;
  return NARDE_OK;
}

int narde_timing_event_destroy(void* event) {
  if (event && hipEventDestroy((hipEvent_t)event) != hipSuccess) return fail(NARDE_EHIP, "hipEventDestroy failed");
  return NARDE_OK;
}

int narde_timing_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return fail(NARDE_EINVAL, "NULL argument");
  if (hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop) != hipSuccess)
    return fail(NARDE_EHIP, "hipEventElapsedTime failed");
  return NARDE_OK;
}

int narde_legal_full(narde_env* e, const uint8_t* dice, uint64_t* legal_first, void* stream) {
  if (!e || !legal_first) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_legal_full<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), dice,
                                                               legal_first);
  return check_launch("k_legal_full");
}

int narde_get_stats(narde_env* e, int32_t* stats, void* stream) {
  if (!e || !stats) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_get_stats<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, stats);
  return check_launch("k_get_stats");
}

int narde_get_totals(narde_env* e, int64_t* rows, void* stream) {
  if (!e || !rows) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_get_totals<<<kTotalRows, kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rows);
  return check_launch("k_get_totals");
}

int narde_apply_moves(narde_env* e, const int8_t* moves, const int8_t* player, void* stream) {
  if (!e || !moves) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_apply<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, moves, player, nullptr);
  return check_launch("k_apply");
}

int narde_observe(narde_env* e, int32_t* obs, float* tes, void* stream) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  if (!obs && !tes) return NARDE_OK;
  if (tes && e->n * 198 >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "too many envs for one observation launch");
  DeviceGuard dg(e->device);
  if (obs) {
    k_observe<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, obs);
    if (const int rc = check_launch("k_observe")) return rc;
  }
  if (tes) {
    // kTesEnvs envs per wave, kBlock / 64 waves per workgroup
    const int64_t per_block = (int64_t)kTesEnvs * (kBlock / 64);
    k_tesauro198_rows<<<(unsigned)((e->n + per_block - 1) / per_block), kBlock, 0, (hipStream_t)stream>>>(
        e->pl, (int)e->n, tes);
    return check_launch("k_tesauro198_rows");
  }
  return NARDE_OK;
}

int narde_dqn_transition(narde_env* e, float* state, const int64_t* actions, const int32_t* reward,
                         const uint8_t* terminated, const uint8_t* truncated, const uint64_t* legal,
                         int32_t* misc, float* off_seen, int shaping, float* r_obs, int64_t* r_action,
                         float* r_reward, float* r_done, float* r_prio, const float* max_prio, const int64_t* pos,
                         int64_t capacity, void* stream) {
  if (!e || !state || !actions || !reward || !terminated || !truncated || !misc || !r_obs || !r_action ||
      !r_reward || !r_done || !r_prio || !max_prio || !pos || (shaping && !off_seen))
    return fail(NARDE_EINVAL, "NULL argument");
  if (capacity < 2 * e->n) return fail(NARDE_EINVAL, "replay capacity below twice the env count");
  if (e->n * 198 >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "too many envs for one transition launch");
  DeviceGuard dg(e->device);
  TransArgs t{e->pl, (int)e->n, shaping, state, actions, reward, terminated, truncated, legal, misc, off_seen,
              r_obs, r_action, r_reward, r_done, r_prio, max_prio, pos, capacity};
  const int64_t per_block = (int64_t)kTesEnvs * (kBlock / 64);  // s' rows per obs workgroup
  const int obs_blocks = (int)((e->n + per_block - 1) / per_block);
  k_dqn_transition<<<(unsigned)(obs_blocks + grid(e->n)), kBlock, 0, (hipStream_t)stream>>>(t, obs_blocks);
  return check_launch("k_dqn_transition");
}

int narde_legal_mask576(narde_env* e, uint64_t* mask, void* stream) {
  if (!e || !mask) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_mask576<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), mask);
  return check_launch("k_mask576");
}

int narde_legal_mask576_move2(narde_env* e, const int16_t* move1, const uint8_t* dice, uint64_t* mask,
                              void* stream) {
  if (!e || !move1 || !mask) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  k_mask576_move2<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), move1, dice,
                                                                  mask);
  return check_launch("k_mask576_move2");
}

int narde_play_set(narde_env* e, const uint8_t* dice, int kind, uint64_t* legal, uint32_t* table, int32_t* count,
                   void* stream) {
  if (!e || !table || !count) return fail(NARDE_EINVAL, "NULL argument");
  if (kind != kPlayAct && kind != kPlayStep) return fail(NARDE_EINVAL, "kind must be 0 (act) or 1 (step)");
  DeviceGuard dg(e->device);
  k_play_set<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), dice, kind, legal, table,
                                                             count);
  return check_launch("k_play_set");
}

int narde_act_masks(narde_env* e, const uint8_t* dice, const int64_t* move1, int64_t ld_move1, uint64_t* mask,
                    void* stream) {
  if (!e || !mask) return fail(NARDE_EINVAL, "NULL argument");
  if (move1 && ld_move1 < 1) return fail(NARDE_EINVAL, "bad move1 stride");
  DeviceGuard dg(e->device);
  k_act_masks<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), dice, move1, ld_move1,
                                                              mask);
  return check_launch("k_act_masks");
}

int narde_explore_plays(narde_env* e, const uint8_t* dice, const float* epsilon, uint64_t seed, const int64_t* tag,
                        int64_t* out, int64_t ld_out, void* stream) {
  if (!e || !epsilon || !tag || !out) return fail(NARDE_EINVAL, "NULL argument");
  if (ld_out < 2) return fail(NARDE_EINVAL, "action rows hold two codes (ld_out >= 2)");
  DeviceGuard dg(e->device);
  k_explore_plays<<<grid(e->n), kBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, rng_of(e), dice, epsilon, tag,
                                                                  (uint32_t)seed, (uint32_t)(seed >> 32), out,
                                                                  ld_out);
  return check_launch("k_explore_plays");
}

int narde_afterstates(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* row_env,
                      int16_t* codes, float* feat, int32_t* obs, int8_t* reward, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, kAftMaxPlays, feat, obs, codes, 4,
                                  "feat and obs must be 16-B aligned, codes 4-B aligned"))
    return rc;
  DeviceGuard dg(e->device);
  return expand_plays(e, AftArgs{e->pl, (int)e->n, rng_of(e), dice, cap, offsets, row_env, codes, feat, obs, reward},
                      nullptr, (hipStream_t)stream);
}

int narde_afterstates_scored(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* row_env,
                             int16_t* codes, int8_t* reward, const narde_value_mlp* net, int perspective,
                             float* value, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, kAftMaxPlays, nullptr, nullptr, codes, 4,
                                  "codes must be 4-B aligned"))
    return rc;
  ValNet vn;
  if (const int rc = check_value_net(net, perspective, value, vn)) return rc;
  DeviceGuard dg(e->device);
  return expand_plays(e, AftArgs{e->pl, (int)e->n, rng_of(e), dice, cap, offsets, row_env, codes, nullptr, nullptr,
                                 reward},
                      &vn, (hipStream_t)stream);
}

int narde_afterstates_lookahead(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* row_env,
                                int16_t* codes, int8_t* reward, const narde_value_mlp* net, int perspective,
                                float* value, void* scratch, int64_t scratch_bytes, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, kAftMaxPlays, nullptr, nullptr, codes, 4,
                                  "codes must be 4-B aligned"))
    return rc;
  ValNet vn;
  if (const int rc = check_value_net(net, perspective, value, vn)) return rc;
  if (perspective != 1) return fail(NARDE_EINVAL, "perspective must be 1 (white's values)");
  if (!scratch) return fail(NARDE_EINVAL, "NULL argument");
  // (32 x cap overflows for no cap a caller can hold rows for: compare in rows)
  if (scratch_bytes < 0 || scratch_bytes / 32 < cap)
    return fail(NARDE_EINVAL, "scratch_bytes %lld below NARDE_LOOKAHEAD_SCRATCH_BYTES = 32 x cap %lld",
                (long long)scratch_bytes, (long long)cap);
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  DeviceGuard dg(e->device);
  hipStream_t st = (hipStream_t)stream;
  const AftArgs a{e->pl, (int)e->n, rng_of(e), dice, cap, offsets, row_env, codes, nullptr, nullptr, reward};
  const int cw = kAftCountBlock / 64, fw = kAftFillBlock / 64;
  k_aft_count<<<(unsigned)((e->n + cw - 1) / cw), kAftCountBlock, 0, st>>>(a);
  if (const int rc = check_launch("k_aft_count")) return rc;
  k_aft_scan<<<1, kAftScanBlock, 0, st>>>(offsets, (int)e->n);
  if (const int rc = check_launch("k_aft_scan")) return rc;
  if (cap == 0) return NARDE_OK;
  k_aft_fill_rec<<<(unsigned)((e->n + fw - 1) / fw), kAftFillBlock, 0, st>>>(a, AftRec{(uint4*)scratch, value});
  if (const int rc = check_launch("k_aft_fill_rec")) return rc;
  // over cap rows (the count is on the device), never more than the rows B envs can have
  const int64_t bound = e->n * (int64_t)kAftMaxPlays;
  const int64_t rows = cap < bound ? cap : bound;
  const LookArgs la{(const uint4*)scratch, offsets, (int)e->n, cap, e->dice_mode};
  if (rows <= kLookSplitRows)  // a short launch: a row's rolls over kLookSplit waves (the same bits)
    k_aft_look<kLookSplit><<<(unsigned)rows, 64 * kLookSplit, 0, st>>>(la, vn);
  else
    k_aft_look<1><<<(unsigned)rows, 64, 0, st>>>(la, vn);
  return check_launch("k_aft_look");
}

int narde_records_lookahead(narde_env* e, int64_t n, const void* records, const narde_value_mlp* net, float* value,
                            void* stream) {
  ValNet vn;
  if (const int rc = check_records_lookahead(e, n, records, net, value, vn)) return rc;
  DeviceGuard dg(e->device);
  hipStream_t st = (hipStream_t)stream;
  // the look kernel reads the caller's records: rows = n, no offsets
  const LookArgs la{(const uint4*)records, nullptr, (int)n, n, e->dice_mode};
  if (n <= kLookSplitRows)  // a short launch, as narde_afterstates_lookahead's (the same bits)
    k_aft_look<kLookSplit, true><<<(unsigned)n, 64 * kLookSplit, 0, st>>>(la, vn);
  else
    k_aft_look<1, true><<<(unsigned)n, 64, 0, st>>>(la, vn);
  return check_launch("k_aft_look<given>");
}

int narde_afterstate_pick(narde_env* e, const int32_t* offsets, const int16_t* codes, int64_t cap,
                          const float* value, int64_t ld_value, int perspective, const float* epsilon,
                          uint64_t seed, const int64_t* tag, int16_t* actions, int32_t* row, void* stream) {
  // a row's two codes are one 32-bit word; no row: (0, 0)
  return pick_rows<uint32_t, 0>(e, offsets, codes, cap, value, ld_value, perspective, epsilon, seed, tag, actions,
                                 row, stream, "k_aft_pick", "codes and actions must be 4-B aligned");
}

namespace {

// What the value rollouts and the league rollouts check alike, in two parts
// (each call's own checks go between them): the handle and the plies; the
// explore pair and the action column (`align`-byte words; misaligned: the
// error's text)
int check_rollout_handle(const narde_env* e, int plies) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  if (plies < 1) return fail(NARDE_EINVAL, "plies %d below 1", plies);
  return NARDE_OK;
}
int check_rollout_columns(const float* epsilon, const int64_t* tag, const void* column, unsigned align,
                          const char* misaligned) {
  if ((epsilon != nullptr) != (tag != nullptr)) return fail(NARDE_EINVAL, "epsilon and tag go together");
  if (reinterpret_cast<uintptr_t>(column) % align) return fail(NARDE_EINVAL, "%s", misaligned);
  return NARDE_OK;
}

// The value rollouts' (narde_value_rollout, narde_turn_value_rollout) checks,
// and the kernels' view of the two nets (the kernels store no per-row value: a
// net's value pointer stays NULL)
int check_rollout_nets(const narde_env* e, int plies, const narde_value_mlp* net_white,
                       const narde_value_mlp* net_black, const float* epsilon, const int64_t* tag, const void* column,
                       unsigned align, const char* misaligned, ValNet& vw, ValNet& vb) {
  if (const int rc = check_rollout_handle(e, plies)) return rc;
  if (!net_white && !net_black)
    return fail(NARDE_EINVAL, "no net for either colour: random play against itself is narde_selfplay");
  if (const int rc = check_rollout_columns(epsilon, tag, column, align, misaligned)) return rc;
  if (net_white)
    if (const int rc = check_value_mlp(net_white, 1, nullptr, kValLdMax, vw)) return rc;
  if (net_black)
    if (const int rc = check_value_mlp(net_black, 1, nullptr, kValLdMax, vb)) return rc;
  return NARDE_OK;
}

// The FULL4 rollouts' and playout's slab: how many waves' pieces it holds
int check_turn_scratch(const void* scratch, int64_t scratch_bytes, int64_t& pieces) {
  if (!scratch) return fail(NARDE_EINVAL, "NULL scratch");
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  pieces = scratch_bytes < 0 ? 0 : scratch_bytes / NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1);
  if (pieces < 1)
    return fail(NARDE_EINVAL, "scratch_bytes %lld below one wave's piece, NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1) = %lld",
                (long long)scratch_bytes, (long long)NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1));
  return NARDE_OK;
}

// the rollout kernels' arguments of a call (two-net and league alike)
VrArgs vr_args(const narde_env* e, int plies, const float* epsilon, uint64_t seed, const int64_t* tag, uint8_t* dice,
               int16_t* actions, float* value, int32_t* reward, uint8_t* terminated, uint8_t* truncated,
               void* records) {
  return VrArgs{e->pl,  (int)e->n,        rng_of(e), e->max_steps, plies,  epsilon,    tag,      (uint32_t)seed,
                (uint32_t)(seed >> 32), dice,      actions,      value,  reward,     terminated, truncated,
                (uint4*)records};
}
TvrArgs tvr_args(const narde_env* e, int plies, const float* epsilon, uint64_t seed, const int64_t* tag, uint8_t* dice,
                 int8_t* play, float* value, int32_t* reward, uint8_t* terminated, uint8_t* truncated, void* scratch,
                 void* records) {
  return TvrArgs{e->pl,      (int)e->n, rng_of(e), e->max_steps, plies,      epsilon,   tag, (uint32_t)seed,
                 (uint32_t)(seed >> 32), dice, reinterpret_cast<uint64_t*>(play), value, reward, terminated,
                 truncated, (uint8_t*)scratch, (uint4*)records};
}

}  // namespace

int narde_value_rollout_records(narde_env* e, int plies, const narde_value_mlp* net_white,
                                const narde_value_mlp* net_black, const float* epsilon, uint64_t seed,
                                const int64_t* tag, uint8_t* dice, int16_t* actions, float* value, int32_t* reward,
                                uint8_t* terminated, uint8_t* truncated, void* records, void* stream) {
  ValNet vw{}, vb{};
  if (const int rc = check_rollout_nets(e, plies, net_white, net_black, epsilon, tag, actions, 4,
                                        "actions must be 4-B aligned", vw, vb))
    return rc;
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  DeviceGuard dg(e->device);
  const VrArgs a = vr_args(e, plies, epsilon, seed, tag, dice, actions, value, reward, terminated, truncated, records);
  return launch_rollout(records != nullptr, k_value_rollout<true>, k_value_rollout<false>, e->n, stream,
                        "k_value_rollout", a, vw, vb, (int)(net_white != nullptr), (int)(net_black != nullptr));
}

int narde_value_rollout(narde_env* e, int plies, const narde_value_mlp* net_white, const narde_value_mlp* net_black,
                        const float* epsilon, uint64_t seed, const int64_t* tag, uint8_t* dice, int16_t* actions,
                        float* value, int32_t* reward, uint8_t* terminated, uint8_t* truncated, void* stream) {
  return narde_value_rollout_records(e, plies, net_white, net_black, epsilon, seed, tag, dice, actions, value, reward,
                                     terminated, truncated, nullptr, stream);
}

int narde_turn_value_rollout_waves(const narde_env* e, int* waves) {
  if (!e || !waves) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  hipDeviceProp_t prop;
  int per_cu = 0;
  hipError_t err = hipGetDeviceProperties(&prop, e->device);
  if (err == hipSuccess)
    err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_turn_value_rollout<false>, 64, 0);
  if (err != hipSuccess) return fail(NARDE_EHIP, "k_turn_value_rollout occupancy: %s", hipGetErrorString(err));
  *waves = prop.multiProcessorCount * per_cu;
  return NARDE_OK;
}

int narde_turn_value_rollout_records(narde_env* e, int plies, const narde_value_mlp* net_white,
                                     const narde_value_mlp* net_black, const float* epsilon, uint64_t seed,
                                     const int64_t* tag, uint8_t* dice, int8_t* play, float* value, int32_t* reward,
                                     uint8_t* terminated, uint8_t* truncated, void* scratch, int64_t scratch_bytes,
                                     void* records, void* stream) {
  ValNet vw{}, vb{};
  if (const int rc = check_rollout_nets(e, plies, net_white, net_black, epsilon, tag, play, 8,
                                        "play must be 8-B aligned", vw, vb))
    return rc;
  int64_t pieces;
  if (const int rc = check_turn_scratch(scratch, scratch_bytes, pieces)) return rc;
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  DeviceGuard dg(e->device);
  const TvrArgs a =
      tvr_args(e, plies, epsilon, seed, tag, dice, play, value, reward, terminated, truncated, scratch, records);
  return launch_rollout(records != nullptr, k_turn_value_rollout<true>, k_turn_value_rollout<false>,
                        pieces < e->n ? pieces : e->n, stream, "k_turn_value_rollout", a, vw, vb,
                        (int)(net_white != nullptr), (int)(net_black != nullptr));
}

int narde_turn_value_rollout(narde_env* e, int plies, const narde_value_mlp* net_white,
                             const narde_value_mlp* net_black, const float* epsilon, uint64_t seed, const int64_t* tag,
                             uint8_t* dice, int8_t* play, float* value, int32_t* reward, uint8_t* terminated,
                             uint8_t* truncated, void* scratch, int64_t scratch_bytes, void* stream) {
  return narde_turn_value_rollout_records(e, plies, net_white, net_black, epsilon, seed, tag, dice, play, value, reward,
                                          terminated, truncated, scratch, scratch_bytes, nullptr, stream);
}

// ---------------------------------------------------------------- leagues
static_assert(kLeagueBatch <= 64 && NARDE_LEAGUE_NETS_MAX % kLeagueBatch == 0, "k_net_table_write's batches");

int narde_net_table(int device, int n_nets, const narde_value_mlp* nets, void* table, int64_t table_bytes,
                    void* stream) {
  if (device < 0) return fail(NARDE_EINVAL, "device %d is negative", device);
  if (!nets || !table) return fail(NARDE_EINVAL, "NULL argument");
  if (n_nets < 1 || n_nets > NARDE_LEAGUE_NETS_MAX)
    return fail(NARDE_EINVAL, "n_nets %d outside 1..%d", n_nets, NARDE_LEAGUE_NETS_MAX);
  if (!aligned16(table)) return fail(NARDE_EINVAL, "table must be 16-B aligned");
  if (table_bytes < NARDE_LEAGUE_TABLE_BYTES(n_nets))
    return fail(NARDE_EINVAL, "table_bytes %lld below NARDE_LEAGUE_TABLE_BYTES(%d) = %lld", (long long)table_bytes,
                n_nets, (long long)NARDE_LEAGUE_TABLE_BYTES(n_nets));
  for (int i = 0; i < n_nets; ++i) {
    ValNet vn;
    if (const int rc = check_value_mlp(&nets[i], 1, nullptr, kValLdMax, vn)) {
      char why[sizeof g_err];
      snprintf(why, sizeof why, "%s", g_err);
      return fail(rc, "net %d: %.400s", i, why);
    }
  }
  DeviceGuard dg(device);
  for (int i0 = 0; i0 < n_nets; i0 += kLeagueBatch) {
    const int count = n_nets - i0 < kLeagueBatch ? n_nets - i0 : kLeagueBatch;
    LeagueBatch b{};
    for (int j = 0; j < count; ++j) {
      const narde_value_mlp& m = nets[i0 + j];
      b.n[j] = LeagueNet{m.w1t, m.ld_w1t, m.b1, m.w2, m.b2, m.hidden, m.hidden_act, m.out_act, 0};
    }
    k_net_table_write<<<1, 64, 0, (hipStream_t)stream>>>(b, count, static_cast<LeagueNet*>(table) + i0);
    if (const int rc = check_launch("k_net_table_write")) return rc;
  }
  return NARDE_OK;
}

namespace {

// The league rollouts' (narde_value_rollout_league,
// narde_turn_value_rollout_league) checks: check_rollout_nets' with the table
// and the two index arrays in place of the nets
int check_league(const narde_env* e, int plies, const void* table, int n_nets, const int32_t* white,
                 const int32_t* black, const float* epsilon, const int64_t* tag, const void* column, unsigned align,
                 const char* misaligned) {
  if (const int rc = check_rollout_handle(e, plies)) return rc;
  if (!table || !white || !black) return fail(NARDE_EINVAL, "NULL argument");
  if (!aligned16(table)) return fail(NARDE_EINVAL, "table must be 16-B aligned");
  if ((reinterpret_cast<uintptr_t>(white) | reinterpret_cast<uintptr_t>(black)) & 3u)
    return fail(NARDE_EINVAL, "white and black must be 4-B aligned");
  if (n_nets < 1 || n_nets > NARDE_LEAGUE_NETS_MAX)
    return fail(NARDE_EINVAL, "n_nets %d outside 1..%d", n_nets, NARDE_LEAGUE_NETS_MAX);
  return check_rollout_columns(epsilon, tag, column, align, misaligned);
}

}  // namespace

int narde_value_rollout_league(narde_env* e, int plies, const void* table, int n_nets, const int32_t* white,
                               const int32_t* black, const float* epsilon, uint64_t seed, const int64_t* tag,
                               uint8_t* dice, int16_t* actions, float* value, int32_t* reward, uint8_t* terminated,
                               uint8_t* truncated, void* records, void* stream) {
  if (const int rc = check_league(e, plies, table, n_nets, white, black, epsilon, tag, actions, 4,
                                  "actions must be 4-B aligned"))
    return rc;
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  DeviceGuard dg(e->device);
  const VrArgs a = vr_args(e, plies, epsilon, seed, tag, dice, actions, value, reward, terminated, truncated, records);
  const LeagueArgs lg{static_cast<const LeagueNet*>(table), n_nets, white, black};
  return launch_rollout(records != nullptr, k_value_rollout_league<true>, k_value_rollout_league<false>, e->n, stream,
                        "k_value_rollout_league", a, lg);
}

int narde_turn_value_rollout_league(narde_env* e, int plies, const void* table, int n_nets, const int32_t* white,
                                    const int32_t* black, const float* epsilon, uint64_t seed, const int64_t* tag,
                                    uint8_t* dice, int8_t* play, float* value, int32_t* reward, uint8_t* terminated,
                                    uint8_t* truncated, void* scratch, int64_t scratch_bytes, void* records,
                                    void* stream) {
  if (const int rc = check_league(e, plies, table, n_nets, white, black, epsilon, tag, play, 8,
                                  "play must be 8-B aligned"))
    return rc;
  int64_t pieces;
  if (const int rc = check_turn_scratch(scratch, scratch_bytes, pieces)) return rc;
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  DeviceGuard dg(e->device);
  const TvrArgs a =
      tvr_args(e, plies, epsilon, seed, tag, dice, play, value, reward, terminated, truncated, scratch, records);
  const LeagueArgs lg{static_cast<const LeagueNet*>(table), n_nets, white, black};
  return launch_rollout(records != nullptr, k_turn_value_rollout_league<true>, k_turn_value_rollout_league<false>,
                        pieces < e->n ? pieces : e->n, stream, "k_turn_value_rollout_league", a, lg);
}

int narde_state_records(int device, int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* first_turn,
                        const int8_t* player, uint32_t t, void* records, void* stream) {
  if (!board || !off || !first_turn || !player || !records) return fail(NARDE_EINVAL, "NULL argument");
  if (n < 1 || n >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "n %lld outside 1 .. 2^31 - 1", (long long)n);
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  DeviceGuard dg(device);
  k_state_records<<<grid(n), kBlock, 0, (hipStream_t)stream>>>(n, board, off, first_turn, player, t, (uint4*)records);
  return check_launch("k_state_records");
}

namespace {

// The playouts' (narde_value_playout, narde_turn_value_playout) checks, and
// the kernels' arguments (the slab is the FULL4 call's own)
int check_playout(const narde_env* e, int64_t n, const void* roots, int trials, int max_plies,
                  const narde_value_mlp* net_white, const narde_value_mlp* net_black, uint64_t seed, int64_t id_base,
                  int flags, int32_t* sums, int8_t* outcome, int32_t* length, float* leaf, VpArgs& a, ValNet& vw,
                  ValNet& vb) {
  if (!e || !roots || !sums) return fail(NARDE_EINVAL, "NULL argument");
  if (n < 1 || trials < 1 || max_plies < 1)
    return fail(NARDE_EINVAL, "n %lld, trials %d and max_plies %d must all be at least 1", (long long)n, trials,
                max_plies);
  constexpr int64_t k31 = int64_t(1) << 31;
  if (n >= k31 || n * (int64_t)trials >= k31)
    return fail(NARDE_EINVAL, "n x trials must stay below 2^31 (n %lld, trials %d)", (long long)n, trials);
  if ((int64_t)trials * (int64_t)max_plies >= k31)
    return fail(NARDE_EINVAL, "trials x max_plies must stay below 2^31 (trials %d, max_plies %d)", trials, max_plies);
  if (flags & ~NARDE_PLAYOUT_COMMON_DICE) return fail(NARDE_EINVAL, "unknown flags 0x%x", (unsigned)flags);
  if (!aligned16(roots)) return fail(NARDE_EINVAL, "roots must be 16-B aligned");
  if (id_base < 0 || id_base + n * (int64_t)trials >= (int64_t(1) << 32))
    return fail(NARDE_EINVAL, "id_base %lld: the trials' env ids must lie in 0 .. 2^32 - 1", (long long)id_base);
  if (!net_white && !net_black)
    return fail(NARDE_EINVAL, "no net for either colour: a playout needs a value net");
  if (net_white)
    if (const int rc = check_value_mlp(net_white, 1, nullptr, kValLdMax, vw)) return rc;
  if (net_black)
    if (const int rc = check_value_mlp(net_black, 1, nullptr, kValLdMax, vb)) return rc;
  a = VpArgs{(const uint4*)roots,
             (int)n,
             trials,
             max_plies,
             Rng{(uint32_t)id_base, (uint32_t)seed, (uint32_t)(seed >> 32), e->dice_mode},
             (flags & NARDE_PLAYOUT_COMMON_DICE) != 0,
             sums,
             outcome,
             length,
             leaf,
             nullptr};
  return NARDE_OK;
}

// sums = 0 ahead of the trials' atomic adds: a kernel of the library's own, not
// hipMemsetAsync -- a captured memset node of this size replayed other bytes
// than zeros under torch.cuda.graph on ROCm 7
int zero_playout_sums(int32_t* sums, int64_t n, hipStream_t stream) {
  k_playout_zero<<<grid(4 * n), kBlock, 0, stream>>>(sums, 4 * n);
  return check_launch("k_playout_zero");
}

}  // namespace

int narde_value_playout(narde_env* e, int64_t n, const void* roots, int trials, int max_plies,
                        const narde_value_mlp* net_white, const narde_value_mlp* net_black, uint64_t seed,
                        int64_t id_base, int flags, int32_t* sums, int8_t* outcome, int32_t* length, float* leaf,
                        void* stream) {
  VpArgs a{};
  ValNet vw{}, vb{};
  if (const int rc = check_playout(e, n, roots, trials, max_plies, net_white, net_black, seed, id_base, flags, sums,
                                   outcome, length, leaf, a, vw, vb))
    return rc;
  DeviceGuard dg(e->device);
  if (const int rc = zero_playout_sums(sums, n, (hipStream_t)stream)) return rc;
  k_value_playout<<<(unsigned)(n * trials), 64, 0, (hipStream_t)stream>>>(a, vw, vb, net_white != nullptr,
                                                                          net_black != nullptr);
  return check_launch("k_value_playout");
}

int narde_turn_value_playout(narde_env* e, int64_t n, const void* roots, int trials, int max_plies,
                             const narde_value_mlp* net_white, const narde_value_mlp* net_black, uint64_t seed,
                             int64_t id_base, int flags, int32_t* sums, int8_t* outcome, int32_t* length, float* leaf,
                             void* scratch, int64_t scratch_bytes, void* stream) {
  VpArgs a{};
  ValNet vw{}, vb{};
  if (const int rc = check_playout(e, n, roots, trials, max_plies, net_white, net_black, seed, id_base, flags, sums,
                                   outcome, length, leaf, a, vw, vb))
    return rc;
  int64_t pieces;
  if (const int rc = check_turn_scratch(scratch, scratch_bytes, pieces)) return rc;
  DeviceGuard dg(e->device);
  const int64_t total = n * trials;
  const int64_t waves = pieces < total ? pieces : total;
  a.slab = (uint8_t*)scratch;
  if (const int rc = zero_playout_sums(sums, n, (hipStream_t)stream)) return rc;
  k_turn_value_playout<<<(unsigned)waves, 64, 0, (hipStream_t)stream>>>(a, vw, vb, net_white != nullptr,
                                                                        net_black != nullptr);
  return check_launch("k_turn_value_playout");
}

int narde_turn_afterstates(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* row_env,
                           int8_t* play, float* feat, int32_t* obs, int8_t* reward, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, NARDE_TURN_AFT_MAX, feat, obs, play, 8,
                                  "feat and obs must be 16-B aligned, play 8-B aligned"))
    return rc;
  DeviceGuard dg(e->device);
  return expand_turns(e, dice, cap, offsets, row_env, play, feat, obs, reward, nullptr, (hipStream_t)stream);
}

int narde_turn_afterstates_scored(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets,
                                  int32_t* row_env, int8_t* play, int8_t* reward, const narde_value_mlp* net,
                                  int perspective, float* value, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, NARDE_TURN_AFT_MAX, nullptr, nullptr, play, 8,
                                  "play must be 8-B aligned"))
    return rc;
  ValNet vn;
  if (const int rc = check_value_net(net, perspective, value, vn)) return rc;
  DeviceGuard dg(e->device);
  return expand_turns(e, dice, cap, offsets, row_env, play, nullptr, nullptr, reward, &vn, (hipStream_t)stream);
}

int narde_turn_afterstates_lookahead(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets,
                                     int32_t* row_env, int8_t* play, int8_t* reward, const narde_value_mlp* net,
                                     int perspective, float* value, void* scratch, int64_t scratch_bytes,
                                     void* stream) {
  if (const int rc = check_expand(e, cap, offsets, NARDE_TURN_AFT_MAX, nullptr, nullptr, play, 8,
                                  "play must be 8-B aligned"))
    return rc;
  ValNet vn;
  if (const int rc = check_value_net(net, perspective, value, vn)) return rc;
  if (perspective != 1) return fail(NARDE_EINVAL, "perspective must be 1 (white's values)");
  if (!scratch) return fail(NARDE_EINVAL, "NULL argument");
  // (128 x cap overflows for no cap a caller can hold rows for: compare in rows)
  if (scratch_bytes < 0 || scratch_bytes / (4 * kTurnLookRowWords) < cap)
    return fail(NARDE_EINVAL, "scratch_bytes %lld below NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES = 128 x cap %lld",
                (long long)scratch_bytes, (long long)cap);
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  DeviceGuard dg(e->device);
  hipStream_t st = (hipStream_t)stream;
  const TurnRec tr{(uint32_t*)scratch, value};
  if (const int rc = expand_turns(e, dice, cap, offsets, row_env, play, nullptr, nullptr, reward, nullptr, st, &tr))
    return rc;
  if (cap == 0) return NARDE_OK;
  // over cap rows (the count is on the device), never more than the rows B envs can have
  const int64_t bound = e->n * (int64_t)NARDE_TURN_AFT_MAX;
  const int64_t rows = cap < bound ? cap : bound;
  const TurnLookArgs la{(uint32_t*)scratch, offsets, (int)e->n, cap, e->dice_mode, e->turn_slab};
  if (rows <= kTurnLookSplitRows)  // a short launch: a row's rolls over kTurnLookSplit waves (the same bits)
    k_turn_look<kTurnLookSplit><<<(unsigned)rows, 64 * kTurnLookSplit, 0, st>>>(la, vn);
  else
    k_turn_look<1><<<(unsigned)rows, 64, 0, st>>>(la, vn);
  if (const int rc = check_launch("k_turn_look")) return rc;
  k_turn_look_overflow<false><<<kTurnOvfWaves, 64, 0, st>>>(la, vn);
  if (const int rc = check_launch("k_turn_look_overflow")) return rc;
  k_turn_look_mean<false>
      <<<(unsigned)((rows + kTurnLookMeanBlock - 1) / kTurnLookMeanBlock), kTurnLookMeanBlock, 0, st>>>(la, value);
  return check_launch("k_turn_look_mean");
}

int narde_turn_records_lookahead(narde_env* e, int64_t n, const void* records, const narde_value_mlp* net,
                                 float* value, void* scratch, int64_t scratch_bytes, void* stream) {
  ValNet vn;
  if (const int rc = check_records_lookahead(e, n, records, net, value, vn)) return rc;
  if (!scratch) return fail(NARDE_EINVAL, "NULL argument");
  if (scratch_bytes < 0 || scratch_bytes / (4 * kTurnLookRowWords) < n)
    return fail(NARDE_EINVAL, "scratch_bytes %lld below NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES = 128 x n %lld",
                (long long)scratch_bytes, (long long)n);
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  DeviceGuard dg(e->device);
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = turn_workspace(e, st)) return rc;  // the overflow pass's slab
  const unsigned lanes = (unsigned)((n + kTurnLookMeanBlock - 1) / kTurnLookMeanBlock);
  k_turn_look_pack<<<lanes, kTurnLookMeanBlock, 0, st>>>((const uint4*)records, n, (uint32_t*)scratch, value);
  if (const int rc = check_launch("k_turn_look_pack")) return rc;
  // the passes of narde_turn_afterstates_lookahead over the n pieces: rows = n, no offsets
  const TurnLookArgs la{(uint32_t*)scratch, nullptr, (int)n, n, e->dice_mode, e->turn_slab};
  if (n <= kTurnLookSplitRows)
    k_turn_look<kTurnLookSplit, true><<<(unsigned)n, 64 * kTurnLookSplit, 0, st>>>(la, vn);
  else
    k_turn_look<1, true><<<(unsigned)n, 64, 0, st>>>(la, vn);
  if (const int rc = check_launch("k_turn_look<given>")) return rc;
  k_turn_look_overflow<true><<<kTurnOvfWaves, 64, 0, st>>>(la, vn);
  if (const int rc = check_launch("k_turn_look_overflow<given>")) return rc;
  k_turn_look_mean<true><<<lanes, kTurnLookMeanBlock, 0, st>>>(la, value);
  return check_launch("k_turn_look_mean<given>");
}

int narde_afterstates_records(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* row_env,
                              int16_t* codes, int8_t* reward, const narde_value_mlp* net, int perspective,
                              float* value, void* records, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, kAftMaxPlays, nullptr, nullptr, codes, 4,
                                  "codes must be 4-B aligned"))
    return rc;
  ValNet vn{};
  if (const int rc = check_records(records, net, perspective, value, vn)) return rc;
  DeviceGuard dg(e->device);
  const AftRec pub{(uint4*)records, nullptr};
  return expand_plays(e, AftArgs{e->pl, (int)e->n, rng_of(e), dice, cap, offsets, row_env, codes, nullptr, nullptr,
                                 reward},
                      net ? &vn : nullptr, (hipStream_t)stream, &pub);
}

int narde_turn_afterstates_records(narde_env* e, const uint8_t* dice, int64_t cap, int32_t* offsets,
                                   int32_t* row_env, int8_t* play, int8_t* reward, const narde_value_mlp* net,
                                   int perspective, float* value, void* records, void* stream) {
  if (const int rc = check_expand(e, cap, offsets, NARDE_TURN_AFT_MAX, nullptr, nullptr, play, 8,
                                  "play must be 8-B aligned"))
    return rc;
  ValNet vn{};
  if (const int rc = check_records(records, net, perspective, value, vn)) return rc;
  DeviceGuard dg(e->device);
  const TurnRec pub{(uint32_t*)records, nullptr};
  return expand_turns(e, dice, cap, offsets, row_env, play, nullptr, nullptr, reward, net ? &vn : nullptr,
                      (hipStream_t)stream, nullptr, &pub);
}

static_assert(kRecordNoneWord6 == NARDE_RECORD_NONE_WORD6, "narde.h and narde_rules.h state the same none record");

int narde_rows_topk(narde_env* e, const int32_t* offsets, int64_t cap, const float* value, int64_t ld_value,
                    int perspective, int k, const void* records, int32_t* sel, void* roots, void* stream) {
  if (!e || !offsets || !value || !sel) return fail(NARDE_EINVAL, "NULL argument");
  if (k < 1 || k > NARDE_TOPK_MAX) return fail(NARDE_EINVAL, "k %d outside 1 .. NARDE_TOPK_MAX = %d", k, NARDE_TOPK_MAX);
  if (perspective != 0 && perspective != 1)
    return fail(NARDE_EINVAL, "perspective must be 0 (the mover's values) or 1 (white's)");
  if (cap < 0) return fail(NARDE_EINVAL, "cap %lld is negative", (long long)cap);
  if (ld_value < 1) return fail(NARDE_EINVAL, "bad value stride");
  if ((roots != nullptr) != (records != nullptr))
    return fail(NARDE_EINVAL, "roots and records must both be set or both be NULL");
  if (!aligned16(roots) || !aligned16(records)) return fail(NARDE_EINVAL, "roots and records must be 16-B aligned");
  if (e->n * (int64_t)k >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "B x k must stay below 2^31 (k %d)", k);
  DeviceGuard dg(e->device);
  const TopkArgs a{e->pl, (int)e->n, offsets, cap, value, ld_value, perspective, k, (const uint4*)records, sel,
                   (uint4*)roots};
  const int w = kTopkBlock / 64;
  k_rows_topk<<<(unsigned)((e->n + w - 1) / w), kTopkBlock, 0, (hipStream_t)stream>>>(a);
  return check_launch("k_rows_topk");
}

int narde_playout_pick(narde_env* e, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld_value,
                       const int8_t* reward, const int16_t* codes, int trials, const int32_t* sums, const float* leaf,
                       int16_t* actions, int32_t* row, float* score, void* stream) {
  return playout_pick_rows<uint32_t, 0>(e, k, sel, cap, value, ld_value, reward, codes, trials, sums, leaf, actions,
                                        row, score, stream, "codes and actions must be 4-B aligned");
}

int narde_turn_playout_pick(narde_env* e, int k, const int32_t* sel, int64_t cap, const float* value,
                            int64_t ld_value, const int8_t* reward, const int8_t* play, int trials,
                            const int32_t* sums, const float* leaf, int8_t* out_play, int32_t* row, float* score,
                            void* stream) {
  return playout_pick_rows<uint64_t, -1>(e, k, sel, cap, value, ld_value, reward, play, trials, sums, leaf, out_play,
                                         row, score, stream, "play and out_play must be 8-B aligned");
}

int narde_slot_pick(narde_env* e, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld_value,
                    const int8_t* reward, const int16_t* codes, const float* slot_score, int16_t* actions,
                    int32_t* row, float* score, void* stream) {
  return slot_pick_rows<uint32_t, 0>(e, k, sel, cap, value, ld_value, reward, codes, slot_score, actions, row, score,
                                     stream, "codes and actions must be 4-B aligned");
}

int narde_turn_slot_pick(narde_env* e, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld_value,
                         const int8_t* reward, const int8_t* play, const float* slot_score, int8_t* out_play,
                         int32_t* row, float* score, void* stream) {
  return slot_pick_rows<uint64_t, -1>(e, k, sel, cap, value, ld_value, reward, play, slot_score, out_play, row, score,
                                      stream, "play and out_play must be 8-B aligned");
}

int narde_value_td_trace(narde_env* e, const narde_value_mlp_train* net, float decay, float* trace, int64_t ld_trace,
                         float* v, uint8_t* black, void* stream) {
  TdNet tn;
  if (const int rc = check_td(e, net, trace, ld_trace, v, black, tn)) return rc;
  DeviceGuard dg(e->device);
  k_td_trace<<<(unsigned)e->n, kTdBlock, 0, (hipStream_t)stream>>>(e->pl, (int)e->n, tn, decay, trace, ld_trace, v,
                                                                    black);
  return check_launch("k_td_trace");
}

int narde_value_td_apply(narde_env* e, const narde_value_mlp_train* net, float* trace, int64_t ld_trace, const float* v,
                         const uint8_t* black, const int32_t* reward, const uint8_t* terminated,
                         const uint8_t* truncated, float alpha, float gamma, int perspective, float* scratch,
                         int64_t scratch_floats, float* delta, void* stream) {
  TdNet tn;
  if (const int rc = check_td(e, net, trace, ld_trace, v, black, tn)) return rc;
  if (!reward || !terminated || !truncated || !scratch) return fail(NARDE_EINVAL, "NULL argument");
  if (perspective != 1) return fail(NARDE_EINVAL, "perspective must be 1 (white's values)");
  const int64_t need = NARDE_TD_SCRATCH_FLOATS(e->n, tn.hidden);
  if (scratch_floats < need)
    return fail(NARDE_EINVAL, "scratch_floats %lld below NARDE_TD_SCRATCH_FLOATS = %lld", (long long)scratch_floats,
                (long long)need);
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  DeviceGuard dg(e->device);
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)e->n, waves = kTdBlock / 64;
  const int slabs = (n + kTdSlab - 1) / kTdSlab;
  const int64_t ld_part = td_row_floats(tn.hidden) + 3;  // (P = 1 mod 4: whole float4 pieces)
  float* dl = scratch;
  float* part = scratch + (e->n + 3) / 4 * 4;
  k_td_delta<<<(unsigned)((n + waves - 1) / waves), kTdBlock, 0, st>>>(e->pl, n, tn, v, black, reward, terminated,
                                                                        truncated, gamma, dl, delta);
  if (const int rc = check_launch("k_td_delta")) return rc;
  const unsigned pieces = (unsigned)((kTdCols / 4) * tn.hidden + 1);  // the float4 pieces and b2's float
  k_td_partial<<<dim3((pieces + kTdBlock - 1) / kTdBlock, (unsigned)slabs), kTdBlock, 0, st>>>(
      n, tn.hidden, trace, ld_trace, dl, terminated, truncated, part, ld_part);
  if (const int rc = check_launch("k_td_partial")) return rc;
  k_td_update<<<(unsigned)((td_row_floats(tn.hidden) + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>(tn, alpha, part,
                                                                                                   ld_part, slabs);
  return check_launch("k_td_update");
}

// narde_value_td_window (the partial rows folded into the weights at step size
// alpha) and narde_value_td_window_grad (folded into grad, no weight written)
static int td_window_call(narde_env* e, const narde_value_mlp_train* net, int plies, const void* records,
                          const int32_t* reward, const uint8_t* terminated, const uint8_t* truncated, float alpha,
                          float lam, float gamma, float* scratch, int64_t scratch_floats, float* delta, bool to_grad,
                          float* grad, void* stream) {
  if (!e || !net || !records || !reward || !terminated || !truncated || !scratch)
    return fail(NARDE_EINVAL, "NULL argument");
  if (to_grad && !grad) return fail(NARDE_EINVAL, "NULL argument");
  if (to_grad && !aligned16(grad)) return fail(NARDE_EINVAL, "grad must be 16-B aligned");
  if (const int rc = check_mlp_fields(net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->hidden, net->hidden_act,
                                      net->out_act, kValLdMax))
    return rc;
  if (net->w1 && net->ld_w1 < 198) return fail(NARDE_EINVAL, "ld_w1 %lld below 198", (long long)net->ld_w1);
  if (plies < 1) return fail(NARDE_EINVAL, "plies %d below 1", plies);
  if (((int64_t)plies + 1) * e->n >= (int64_t(1) << 31))
    return fail(NARDE_EINVAL, "(plies + 1) x B = %lld samples: 2^31 or more", (long long)(((int64_t)plies + 1) * e->n));
  if (!(lam >= 0.0f && lam <= 1.0f)) return fail(NARDE_EINVAL, "lam %g outside [0, 1]", (double)lam);
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  const int64_t need = tdw_scratch_floats(e->n, plies, net->hidden);
  if (scratch_floats < need)
    return fail(NARDE_EINVAL, "scratch_floats %lld below NARDE_TD_WINDOW_SCRATCH_FLOATS = %lld",
                (long long)scratch_floats, (long long)need);
  const TdNet tn{net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->w1, net->ld_w1, net->hidden, net->hidden_act,
                 net->out_act};
  DeviceGuard dg(e->device);
  hipStream_t st = (hipStream_t)stream;
  // k_tdw_grad's accumulator is past the 64 KB a launch may ask for unannounced from hidden = 82 on: once a device
  static std::atomic<uint64_t> announced{0};
  const uint64_t bit = uint64_t(1) << (e->device & 63);
  if (!(announced.load(std::memory_order_relaxed) & bit)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tdw_grad), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(td_row_floats(kValHiddenMax) * sizeof(float))));
    announced.fetch_or(bit, std::memory_order_relaxed);
  }
  const int n = (int)e->n;
  const int64_t stored = (int64_t)plies * n, all = stored + n;
  const int slabs = (int)tdw_slabs(stored);
  const int64_t P = td_row_floats(tn.hidden), ld_part = P + 3;
  float* v = scratch;
  float* G = v + tdw_round4(all);
  float* part = G + tdw_round4(stored);
  k_tdw_values<<<(unsigned)((all + kTdwWaves - 1) / kTdwWaves), kTdBlock, 0, st>>>(e->pl, (const uint4*)records, stored,
                                                                                   all, tn, v);
  if (const int rc = check_launch("k_tdw_values")) return rc;
  k_tdw_returns<<<(unsigned)((n + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>(
      n, plies, (const uint32_t*)records, v, reward, terminated, truncated, gamma, gamma * lam, G, delta);
  if (const int rc = check_launch("k_tdw_returns")) return rc;
  k_tdw_grad<<<(unsigned)slabs, 2 * kTdBlock, (size_t)P * sizeof(float), st>>>((const uint4*)records, stored, tn, G, part,
                                                                           ld_part);
  if (const int rc = check_launch("k_tdw_grad")) return rc;
  if (to_grad) {
    k_td_fold<<<(unsigned)((P + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>((int)P, part, ld_part, slabs, grad);
    return check_launch("k_td_fold");
  }
  k_td_update<<<(unsigned)((P + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>(tn, alpha, part, ld_part, slabs);
  return check_launch("k_td_update");
}

int narde_value_td_window(narde_env* e, const narde_value_mlp_train* net, int plies, const void* records,
                          const int32_t* reward, const uint8_t* terminated, const uint8_t* truncated, float alpha,
                          float lam, float gamma, float* scratch, int64_t scratch_floats, float* delta, void* stream) {
  return td_window_call(e, net, plies, records, reward, terminated, truncated, alpha, lam, gamma, scratch,
                        scratch_floats, delta, false, nullptr, stream);
}

int narde_value_td_window_grad(narde_env* e, const narde_value_mlp_train* net, int plies, const void* records,
                               const int32_t* reward, const uint8_t* terminated, const uint8_t* truncated, float lam,
                               float gamma, float* scratch, int64_t scratch_floats, float* delta, float* grad,
                               void* stream) {
  return td_window_call(e, net, plies, records, reward, terminated, truncated, 0.0f, lam, gamma, scratch,
                        scratch_floats, delta, true, grad, stream);
}

// narde_value_fit and narde_value_fit_grad, as td_window_call
static int value_fit_call(int device, const narde_value_mlp_train* net, int64_t n, const void* records,
                          const float* target, const float* weight, float alpha, float* scratch, int64_t scratch_floats,
                          float* v, double* loss, bool to_grad, float* grad, void* stream) {
  if (!net || !records || !target || !scratch) return fail(NARDE_EINVAL, "NULL argument");
  if (to_grad && !grad) return fail(NARDE_EINVAL, "NULL argument");
  if (to_grad && !aligned16(grad)) return fail(NARDE_EINVAL, "grad must be 16-B aligned");
  if (device < 0) return fail(NARDE_EINVAL, "device %d is negative", device);
  if (const int rc = check_mlp_fields(net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->hidden, net->hidden_act,
                                      net->out_act, kValLdMax))
    return rc;
  if (net->w1 && net->ld_w1 < 198) return fail(NARDE_EINVAL, "ld_w1 %lld below 198", (long long)net->ld_w1);
  if (n < 1 || n >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "n %lld outside 1 .. 2^31 - 1", (long long)n);
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  if (!aligned16(scratch)) return fail(NARDE_EINVAL, "scratch must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(loss) & 7u) return fail(NARDE_EINVAL, "loss must be 8-B aligned");
  const int64_t need = fit_scratch_floats(n, net->hidden);
  if (scratch_floats < need)
    return fail(NARDE_EINVAL, "scratch_floats %lld below NARDE_VALUE_FIT_SCRATCH_FLOATS = %lld",
                (long long)scratch_floats, (long long)need);
  const TdNet tn{net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->w1, net->ld_w1, net->hidden, net->hidden_act,
                 net->out_act};
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  // k_fit_grad's accumulator, as k_tdw_grad's, is past the 64 KB a launch may ask for unannounced from hidden = 82
  // on: once a device
  static std::atomic<uint64_t> announced{0};
  const uint64_t bit = uint64_t(1) << (device & 63);
  if (!(announced.load(std::memory_order_relaxed) & bit)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fit_grad), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(td_row_floats(kValHiddenMax) * sizeof(float))));
    announced.fetch_or(bit, std::memory_order_relaxed);
  }
  const int slabs = (int)tdw_slabs(n);
  const int64_t P = td_row_floats(tn.hidden), ld_part = P + 3;
  float* part = scratch;
  double* slab_loss = reinterpret_cast<double*>(scratch + slabs * ld_part);  // (ld_part: whole float4s)
  k_fit_grad<<<(unsigned)slabs, 2 * kTdBlock, (size_t)P * sizeof(float), st>>>((const uint4*)records, n, tn, target, weight,
                                                                           part, ld_part, slab_loss, v);
  if (const int rc = check_launch("k_fit_grad")) return rc;
  if (to_grad) {
    k_td_fold<<<(unsigned)((P + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>((int)P, part, ld_part, slabs, grad);
    if (const int rc = check_launch("k_td_fold")) return rc;
  } else {
    k_td_update<<<(unsigned)((P + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>(tn, alpha, part, ld_part, slabs);
    if (const int rc = check_launch("k_td_update")) return rc;
  }
  if (!loss) return NARDE_OK;
  k_fit_loss<<<1, 64, 0, st>>>(slab_loss, slabs, loss);
  return check_launch("k_fit_loss");
}

int narde_value_fit(int device, const narde_value_mlp_train* net, int64_t n, const void* records, const float* target,
                    const float* weight, float alpha, float* scratch, int64_t scratch_floats, float* v, double* loss,
                    void* stream) {
  return value_fit_call(device, net, n, records, target, weight, alpha, scratch, scratch_floats, v, loss, false,
                        nullptr, stream);
}

int narde_value_fit_grad(int device, const narde_value_mlp_train* net, int64_t n, const void* records,
                         const float* target, const float* weight, float* scratch, int64_t scratch_floats, float* v,
                         double* loss, float* grad, void* stream) {
  return value_fit_call(device, net, n, records, target, weight, 0.0f, scratch, scratch_floats, v, loss, true, grad,
                        stream);
}

// a trained net's description as the optimiser steps check it, and the kernels' view of it
static int check_opt_net(int device, const narde_value_mlp_train* net, TdNet& tn) {
  if (device < 0) return fail(NARDE_EINVAL, "device %d is negative", device);
  if (!net) return fail(NARDE_EINVAL, "NULL argument");
  if (const int rc = check_mlp_fields(net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->hidden, net->hidden_act,
                                      net->out_act, kValLdMax))
    return rc;
  if (net->w1 && net->ld_w1 < 198) return fail(NARDE_EINVAL, "ld_w1 %lld below 198", (long long)net->ld_w1);
  tn = TdNet{net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->w1, net->ld_w1, net->hidden, net->hidden_act,
             net->out_act};
  return NARDE_OK;
}

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0u; }

int narde_value_grad_norm(int device, int hidden, const float* grad, float max_norm, float* out, void* stream) {
  if (device < 0) return fail(NARDE_EINVAL, "device %d is negative", device);
  if (!grad || !out) return fail(NARDE_EINVAL, "NULL argument");
  if (hidden < 1 || hidden > NARDE_VALUE_HIDDEN_MAX)
    return fail(NARDE_EINVAL, "hidden %d outside 1..%d", hidden, NARDE_VALUE_HIDDEN_MAX);
  if (!aligned16(grad)) return fail(NARDE_EINVAL, "grad must be 16-B aligned");
  if (!aligned4(out)) return fail(NARDE_EINVAL, "out must be 4-B aligned");
  if (!(max_norm >= 0.0f)) return fail(NARDE_EINVAL, "max_norm %g is negative", (double)max_norm);
  DeviceGuard dg(device);
  k_opt_norm<<<1, kOptBlock, 0, (hipStream_t)stream>>>((int)td_row_floats(hidden), grad, max_norm, out);
  return check_launch("k_opt_norm");
}

int narde_value_sgd_step(int device, const narde_value_mlp_train* net, const float* grad, const float* scale,
                         float alpha, void* stream) {
  TdNet tn;
  if (const int rc = check_opt_net(device, net, tn)) return rc;
  if (!grad) return fail(NARDE_EINVAL, "NULL argument");
  if (!aligned16(grad)) return fail(NARDE_EINVAL, "grad must be 16-B aligned");
  if (!aligned4(scale)) return fail(NARDE_EINVAL, "scale must be 4-B aligned");
  if (!(alpha >= 0.0f)) return fail(NARDE_EINVAL, "alpha %g is negative", (double)alpha);
  DeviceGuard dg(device);
  const int64_t P = td_row_floats(tn.hidden);
  k_sgd_step<<<(unsigned)((P + kTdBlock - 1) / kTdBlock), kTdBlock, 0, (hipStream_t)stream>>>(tn, grad, scale, alpha);
  return check_launch("k_sgd_step");
}

int narde_value_adam_step(int device, const narde_value_mlp_train* net, const float* grad, const float* scale,
                          float* m, float* s, narde_adam_state* state, float lr, float beta1, float beta2, float eps,
                          float weight_decay, void* stream) {
  TdNet tn;
  if (const int rc = check_opt_net(device, net, tn)) return rc;
  if (!grad || !m || !s || !state) return fail(NARDE_EINVAL, "NULL argument");
  if (!aligned16(grad) || !aligned16(m) || !aligned16(s)) return fail(NARDE_EINVAL, "grad, m and s must be 16-B aligned");
  if (!aligned4(scale)) return fail(NARDE_EINVAL, "scale must be 4-B aligned");
  if (reinterpret_cast<uintptr_t>(state) & 7u) return fail(NARDE_EINVAL, "state must be 8-B aligned");
  if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f))
    return fail(NARDE_EINVAL, "beta1 %g, beta2 %g: outside [0, 1)", (double)beta1, (double)beta2);
  if (!(eps > 0.0f)) return fail(NARDE_EINVAL, "eps %g is not positive", (double)eps);
  if (!(lr >= 0.0f)) return fail(NARDE_EINVAL, "lr %g is negative", (double)lr);
  if (!(weight_decay >= 0.0f)) return fail(NARDE_EINVAL, "weight_decay %g is negative", (double)weight_decay);
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  AdamState* ds = reinterpret_cast<AdamState*>(state);
  const float keep = 1.0f - lr * weight_decay;
  const int64_t P = td_row_floats(tn.hidden);
  k_adam_tick<<<1, 64, 0, st>>>(ds, beta1, beta2);
  if (const int rc = check_launch("k_adam_tick")) return rc;
  k_adam_step<<<(unsigned)((P + kTdBlock - 1) / kTdBlock), kTdBlock, 0, st>>>(tn, grad, scale, m, s, ds, lr, beta1, beta2,
                                                                             eps, keep);
  return check_launch("k_adam_step");
}

int narde_playout_targets(int device, int64_t n, int trials, const int32_t* sums, const float* leaf, const void* roots,
                          float* target, float* weight, void* stream) {
  if (!sums || !target || !weight) return fail(NARDE_EINVAL, "NULL argument");
  if (device < 0) return fail(NARDE_EINVAL, "device %d is negative", device);
  if (n < 1 || n >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "n %lld outside 1 .. 2^31 - 1", (long long)n);
  if (trials < 1) return fail(NARDE_EINVAL, "trials %d below 1", trials);
  if (n * (int64_t)trials >= (int64_t(1) << 31))
    return fail(NARDE_EINVAL, "n x trials = %lld: 2^31 or more", (long long)(n * (int64_t)trials));
  if (!aligned16(roots)) return fail(NARDE_EINVAL, "roots must be 16-B aligned");
  DeviceGuard dg(device);
  k_playout_targets<<<grid(n), kBlock, 0, (hipStream_t)stream>>>(n, trials, sums, leaf, (const uint32_t*)roots, target,
                                                                 weight);
  return check_launch("k_playout_targets");
}

int narde_turn_pick(narde_env* e, const int32_t* offsets, const int8_t* play, int64_t cap, const float* value,
                    int64_t ld_value, int perspective, const float* epsilon, uint64_t seed, const int64_t* tag,
                    int8_t* out_play, int32_t* row, void* stream) {
  // a row's (4,2) int8 play is one 64-bit word; no row: all -1
  return pick_rows<uint64_t, -1>(e, offsets, play, cap, value, ld_value, perspective, epsilon, seed, tag, out_play,
                                    row, stream, "k_turn_pick", "play and out_play must be 8-B aligned");
}

int narde_policy_masked_argmax576(int device, const float* q, int64_t ldq, const uint64_t* mask, int64_t n,
                                  float epsilon, uint64_t seed, uint32_t tag, int head, int64_t* out,
                                  void* stream) {
  if (!q || !mask || !out || n < 0 || n > (int64_t(1) << 31) - 4 || ldq < 576)
    return fail(NARDE_EINVAL, "bad argument");
  if (n == 0) return NARDE_OK;
  DeviceGuard dg(device);
  k_policy576<<<(int)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(q, ldq, mask, (int)n, eps_to_q32(epsilon),
                                                                   (uint32_t)seed, (uint32_t)(seed >> 32), tag,
                                                                   head, out, nullptr, nullptr, nullptr, 0,
                                                                   nullptr);
  return check_launch("k_policy576");
}

int narde_policy_masked_argmax576_dev(int device, const float* q, int64_t ldq, const uint64_t* mask, int64_t n,
                                      const float* epsilon, uint64_t seed, const int64_t* tag, int head,
                                      const float* add_tab, int64_t ld_add, const int64_t* add_row,
                                      int64_t* out, void* stream) {
  if (!q || !mask || !out || !epsilon || !tag || n < 0 || n > (int64_t(1) << 31) - 4 || ldq < 576)
    return fail(NARDE_EINVAL, "bad argument");
  if (add_tab && (!add_row || ld_add < 576)) return fail(NARDE_EINVAL, "bad addend table");
  if (n == 0) return NARDE_OK;
  DeviceGuard dg(device);
  k_policy576<<<(int)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(q, ldq, mask, (int)n, 0ull, (uint32_t)seed,
                                                                   (uint32_t)(seed >> 32), 0u, head, out, epsilon,
                                                                   tag, add_tab, ld_add, add_row);
  return check_launch("k_policy576");
}

int narde_head_policy576_dev(int device, const float* f, int64_t ldf, int64_t feat, const float* w, int64_t ldw,
                             const float* bias, const uint64_t* mask, int64_t n, const float* epsilon,
                             uint64_t seed, const int64_t* tag, int head, const float* addcol,
                             const int64_t* add_row, int64_t ld_row, int64_t* out, int64_t ld_out,
                             int16_t* out16, int64_t ld_out16, void* stream) {
  if (!f || !w || !bias || !mask || !out || !epsilon || !tag || n < 0 || n > (int64_t(1) << 31) - 4)
    return fail(NARDE_EINVAL, "bad argument");
  if (ld_out < 1 || (out16 && ld_out16 < 1) || (addcol && ld_row < 1)) return fail(NARDE_EINVAL, "bad strides");
  if (feat != kHeadF || ldf < feat || ldw < feat || (ldf % 4) || (ldw % 4) ||
      !aligned16(f) || !aligned16(w))
    return fail(NARDE_EINVAL, "features must be 256 wide, rows 16-B aligned");
  if (addcol && !add_row) return fail(NARDE_EINVAL, "addend column without its rows");
  if (n == 0) return NARDE_OK;
  DeviceGuard dg(device);
  k_head_policy576<<<(int)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(f, ldf, w, ldw, bias, mask, (int)n,
                                                                        (uint32_t)seed, (uint32_t)(seed >> 32),
                                                                        head, out, ld_out, out16, ld_out16,
                                                                        epsilon, tag, addcol, add_row, ld_row);
  return check_launch("k_head_policy576");
}

int narde_violates_block_rule(int device, const int8_t* boards, int64_t n, uint8_t* out, void* stream) {
  if (!boards || !out || n < 0 || n > (int64_t(1) << 31) - kBlock) return fail(NARDE_EINVAL, "bad argument");
  if (n == 0) return NARDE_OK;
  DeviceGuard dg(device);
  k_block<<<grid(n), kBlock, 0, (hipStream_t)stream>>>(boards, (int)n, out);
  return check_launch("k_block");
}

}  // extern "C"

// ------------------------------------------------------- host entry points
namespace {

// One narde_host_* call's staging.  An input has one offset in the pinned and
// the device input buffer, an output one in the two output buffers; every
// array starts on a kStageSlot boundary (the kernels read and write them as
// they do device arrays: 16-byte row stores and the like).  The call declares
// its arrays, then upload(), its launches, download(), and write_back() once
// nothing can refuse the call any more.
class Stage {
 public:
  explicit Stage(narde_env* e) : env(e) {}

  // an input: count elements of the caller's src; returns the device copy
  // (filled by upload())
  template <class T>
  const T* in(const T* src, int64_t count) {
    const size_t at = in_, bytes = (size_t)count * sizeof(T);
    in_ += stage_slot(bytes);
    memcpy(env->h_in + at, src, bytes);
    return reinterpret_cast<const T*>(env->d_in + at);
  }

  // an output: returns the device array of count elements; write_back()
  // copies them to the caller's dst (NULL: to nobody)
  template <class T>
  T* out(T* dst, int64_t count) {
    const size_t at = out_, bytes = (size_t)count * sizeof(T);
    out_ += stage_slot(bytes);
    if (dst) back_[nback_++] = Back{dst, at, bytes};
    return reinterpret_cast<T*>(env->d_out + at);
  }

  int upload() {
    HIP_TRY(hipMemcpyAsync(env->d_in, env->h_in, in_, hipMemcpyHostToDevice, env->hstream));
    return NARDE_OK;
  }

  // the outputs in pinned memory, the stream drained
  int download() {
    HIP_TRY(hipMemcpyAsync(env->h_out, env->d_out, out_, hipMemcpyDeviceToHost, env->hstream));
    HIP_TRY(hipStreamSynchronize(env->hstream));
    return NARDE_OK;
  }

  // a downloaded output, by its device array
  template <class T>
  const T* host(const T* dev) const {
    return reinterpret_cast<const T*>(env->h_out + (reinterpret_cast<const uint8_t*>(dev) - env->d_out));
  }

  void write_back() const {
    for (int k = 0; k < nback_; ++k) memcpy(back_[k].dst, env->h_out + back_[k].at, back_[k].bytes);
  }

 private:
  struct Back { void* dst; size_t at, bytes; };
  narde_env* env;
  size_t in_ = 0, out_ = 0;
  Back back_[kStageArrays];
  int nback_ = 0;
};

// n envs of arrays of these bytes per env, staged; the calls' largest: the
// outputs and the inputs of narde_host_step, narde_host_legal_moves' outputs
constexpr size_t staged(int64_t n, std::initializer_list<int> env_bytes) {
  size_t at = 0;
  for (const int b : env_bytes) at += stage_slot((size_t)n * b);
  return at;
}
static_assert(kStageArrays >= 7 && staged(kHostCap, {24, 2, 2, 1, 24 * 4, 4, 1}) <= kStageBytes &&
                  staged(kHostCap, {24, 2, 2, 1, 2, 2 * 2}) <= kStageBytes &&
                  staged(kHostCap, {2, NARDE_MAX_MOVES * 2}) <= kStageBytes,
              "a narde_host_* call at kHostCap envs exceeds the staging buffers");

int host_check(narde_env* e, int64_t n) {
  if (!e) return fail(NARDE_EINVAL, "NULL handle");
  if (n < 0 || n > kHostCap) return fail(NARDE_EINVAL, "host batch %lld > %lld", (long long)n, (long long)kHostCap);
  return NARDE_OK;
}

int host_validate(int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft, const int8_t* player) {
  for (int64_t i = 0; i < n; ++i)
    if (!valid_position(board, off, ft, player, i))
      return fail(NARDE_EINVAL, "invalid position at index %lld", (long long)i);
  return NARDE_OK;
}

// the position block of n envs, staged in; set(): into the handle's host
// envs, once uploaded
struct PositionIn {
  const int8_t* board;
  const uint8_t *off, *ft;
  const int8_t* player;
  void set(narde_env* e, int64_t n) const {
    k_set_state<<<grid(n), kBlock, 0, e->hstream>>>(e->hpl, (int)n, board, off, ft, player, nullptr, 0);
  }
};

PositionIn stage_position(Stage& st, int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft,
                          const int8_t* player) {
  return PositionIn{st.in(board, n * 24), st.in(off, n * 2), st.in(ft, n * 2), st.in(player, n)};
}

// the host envs' position block read back into the caller's arrays (player
// NULL: not read)
void get_host_state(narde_env* e, Stage& st, int64_t n, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player) {
  int8_t* db = st.out(board, n * 24);
  uint8_t* doff = st.out(off, n * 2);
  uint8_t* dft = st.out(ft, n * 2);
  int8_t* dp = player ? st.out(player, n) : nullptr;
  k_get_state<<<grid(n), kBlock, 0, e->hstream>>>(e->hpl, (int)n, db, doff, dft, dp, nullptr);
}

}  // namespace

extern "C" {

int narde_host_legal_moves(narde_env* e, int64_t n, const int8_t* board, const uint8_t* off,
                           const uint8_t* ft, const int8_t* player, const uint8_t* dice4,
                           int16_t* count, int8_t* moves) {
  int rc = host_check(e, n);
  if (rc) return rc;
  if (n == 0) return NARDE_OK;
  if (!board || !off || !ft || !player || !dice4 || !count) return fail(NARDE_EINVAL, "NULL argument");
  if ((rc = host_validate(n, board, off, ft, player))) return rc;
  DeviceGuard dg(e->device);
  Stage st(e);
  const PositionIn pos = stage_position(st, n, board, off, ft, player);
  const uint8_t* dd = st.in(dice4, n * 4);
  int16_t* dc = st.out(count, n);
  int8_t* dm = st.out(moves, n * NARDE_MAX_MOVES * 2);
  if ((rc = st.upload())) return rc;
  pos.set(e, n);
  k_legal<<<grid(n), kBlock, 0, e->hstream>>>(e->hpl, (int)n, rng_of(e), dd, dc, moves ? dm : nullptr,
                                              nullptr);
  if ((rc = check_launch("host legal"))) return rc;
  if ((rc = st.download())) return rc;
  st.write_back();
  return NARDE_OK;
}

int narde_host_step(narde_env* e, int64_t n, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player,
                    const uint8_t* dice2, const int16_t* actions, int32_t* obs, int32_t* reward,
                    uint8_t* terminated) {
  int rc = host_check(e, n);
  if (rc) return rc;
  if (n == 0) return NARDE_OK;
  if (!board || !off || !ft || !player || !dice2 || !actions) return fail(NARDE_EINVAL, "NULL argument");
  if ((rc = host_validate(n, board, off, ft, player))) return rc;
  for (int64_t i = 0; i < 2 * n; ++i)
    if (dice2[i] < 1 || dice2[i] > 6) return fail(NARDE_EINVAL, "die out of range at %lld", (long long)i);
  DeviceGuard dg(e->device);
  Stage st(e);
  const PositionIn pos = stage_position(st, n, board, off, ft, player);
  const uint8_t* dd = st.in(dice2, n * 2);
  const int16_t* da = st.in(actions, n * 2);
  const Outs out{st.out(obs, n * 24), st.out(reward, n), st.out(terminated, n), nullptr, nullptr, nullptr, nullptr};
  if ((rc = st.upload())) return rc;
  pos.set(e, n);
  k_step<false><<<grid(n), kBlock, 0, e->hstream>>>(step_args(e, e->hpl, n, 0, 0, da, nullptr, dd, out));
  get_host_state(e, st, n, board, off, ft, player);
  if ((rc = check_launch("host step"))) return rc;
  if ((rc = st.download())) return rc;
  st.write_back();
  return NARDE_OK;
}

int narde_host_apply_moves(narde_env* e, int64_t n, int8_t* board, uint8_t* off, uint8_t* ft,
                           const int8_t* player, const int8_t* moves) {
  int rc = host_check(e, n);
  if (rc) return rc;
  if (n == 0) return NARDE_OK;
  if (!board || !off || !ft || !player || !moves) return fail(NARDE_EINVAL, "NULL argument");
  if ((rc = host_validate(n, board, off, ft, player))) return rc;
  DeviceGuard dg(e->device);
  Stage st(e);
  const PositionIn pos = stage_position(st, n, board, off, ft, player);
  const int8_t* dm = st.in(moves, n * 2);
  uint8_t* status = st.out<uint8_t>(nullptr, n);
  if ((rc = st.upload())) return rc;
  pos.set(e, n);
  k_apply<<<grid(n), kBlock, 0, e->hstream>>>(e->hpl, (int)n, dm, pos.player, status);
  get_host_state(e, st, n, board, off, ft, nullptr);
  if ((rc = check_launch("host apply"))) return rc;
  if ((rc = st.download())) return rc;
  // a move the record cannot hold (k_apply): nothing is written back
  const uint8_t* refused = st.host(status);
  for (int64_t i = 0; i < n; ++i)
    if (refused[i])
      return fail(NARDE_EINVAL,
                  "move (%d, %d) at index %lld is not executable: the source holds none of the "
                  "mover's checkers or the target holds opponent checkers",
                  (int)moves[2 * i], (int)moves[2 * i + 1], (long long)i);
  st.write_back();
  return NARDE_OK;
}

int narde_host_violates_block_rule(narde_env* e, int64_t n, const int8_t* boards, uint8_t* out) {
  int rc = host_check(e, n);
  if (rc) return rc;
  if (n == 0) return NARDE_OK;
  if (!boards || !out) return fail(NARDE_EINVAL, "NULL argument");
  DeviceGuard dg(e->device);
  Stage st(e);
  const int8_t* db = st.in(boards, n * 24);
  uint8_t* dr = st.out(out, n);
  if ((rc = st.upload())) return rc;
  k_block<<<grid(n), kBlock, 0, e->hstream>>>(db, (int)n, dr);
  if ((rc = check_launch("host block"))) return rc;
  if ((rc = st.download())) return rc;
  st.write_back();
  return NARDE_OK;
}

}  // extern "C"
