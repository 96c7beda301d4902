// kernels_turn_afterstates.h -- FULL4 whole-turn afterstates: the level walk
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_rows.h: the row set, the scan, the pick and the wave
// helpers are there); not a standalone header.
#pragma once

namespace {

// A wave per env (narde_rules.h "FULL4 turn afterstates" gives the
// semantics).  The frontier -- the distinct positions of a level, each a
// path word -- lives in two buffers that swap from level to level; the exact
// 41-bit keys are kept for the level being built only (nothing reads a
// finished level's keys).  A level is expanded 64 parents at a time:
//   1. lane = parent: the root with the path applied (turn_path_apply), its
//      sub-move lists (turn_node_lists: legal1 with the turn's one low mask,
//      block-free turns skip the block filter) and a wave prefix sum of the
//      list lengths;
//   2. the children go 64 per chunk, lane = child: the lane finds its parent
//      in the prefix sums (6-step search in LDS), builds the child's path and
//      key (turn_child, turn_path_key), and compares the key with the kept
//      nodes of the next level (two keys a 16-B read) and with the earlier
//      lanes of its own chunk (v_readlane);
//   3. a ballot of the survivors and a popcount below the lane give each its
//      slot: a level is in enumeration order with no atomics.
// The count pass stops at the deepest non-empty level (the env's count ->
// offsets[e + 1], then k_aft_scan); the fill pass also carries out every
// node of that level, writes its narrow outputs from the lane, and streams
// the 198-float rows through LDS (aft_flush_feat, as k_aft_fill).
//
// Frontier size: in random play an env has 15 rows on average and no level
// above 256 nodes on 99.97 % of turns; the proven bound is kTurnAftMax =
// 5,220.  The
// fast kernels keep kTurnFront nodes a level in LDS; an env whose level
// outgrows that is appended to a device-side list (the order of the list is
// the only thing an atomic decides: every env's rows and their place are
// its own) and redone by a second, fixed-grid launch (k_turn_overflow) with
// 2,048 nodes a level in LDS and, past that, a handle-owned slab of
// kTurnAftMax nodes a level per wave -- nothing synchronises, every env is
// exact.
static_assert(kTurnAftMax == NARDE_TURN_AFT_MAX, "narde.h and narde_rules.h state the same bound");
constexpr int kTurnFront = 256;      // fast path: nodes a level
constexpr int kTurnCountBlock = 256;  // count pass: 4 envs per workgroup (19.3 KiB of LDS)
constexpr int kTurnFillBlock = 64;    // fill pass: an env per workgroup (13.2 KiB of LDS)
constexpr int kTurnOvfWaves = 128;    // overflow launches: workgroups of one wave, grid-stride over the list
// slab bytes per overflow wave: a level of keys (+ 2 sentinels) and two of paths
constexpr size_t kTurnSlabKeys = (size_t)kTurnAftMax + 2;
constexpr size_t kTurnSlabWave = kTurnSlabKeys * sizeof(uint64_t) + 2 * (size_t)kTurnAftMax * sizeof(uint32_t);
static_assert(kTurnSlabWave % 16 == 0, "every wave's keys are read 16 B at a time");

struct TurnArgs {
  Planes pl;
  int n;
  Rng g;
  const uint8_t* __restrict__ dice;
  int64_t cap;
  int32_t* __restrict__ offsets;  // [n + 1]
  int32_t* __restrict__ row_env;  // [cap]
  int8_t* __restrict__ play;      // [cap][4][2]
  float* __restrict__ feat;       // [cap][198]
  int32_t* __restrict__ obs;      // [cap][24]
  int8_t* __restrict__ reward;    // [cap]
  int32_t* __restrict__ ovf;      // [1 + n]: the overflow envs' count, then the envs
  uint8_t* __restrict__ slab;     // [kTurnOvfWaves][kTurnSlabWave]
};

struct alignas(16) TurnScan {  // per wave: the 64 parents of a chunk
  uint32_t incl[64];  // inclusive prefix sums of their child counts
  uint32_t w0[64];    // their lists (turn_node_lists)
  uint32_t w1[64];
};

struct alignas(16) TurnFrontLds {  // per wave, fast path
  uint64_t key[kTurnFront + 2];  // the level being built; kTurnNoKey behind the last (two a read)
  uint32_t path[2][kTurnFront];
};

// What the record fill (kernels_turn_lookahead.h) writes besides the narrow
// outputs: row R's 128-B piece of the lookahead's scratch -- the record after
// the turn, its ply-counter word replaced by the reward (the later passes
// read it as "terminal"), and the word of rolls to redo cleared -- and a
// terminal row's outcome in white's perspective.
constexpr int kTurnLookRowWords = 32;   // 128 B a row
constexpr int kTurnLookBest = 8;        // word 8 .. 28: the 21 unordered rolls' bests
constexpr int kTurnLookRedo = 29;       // word 29: bit k = roll k outgrew the fast frontier
struct TurnRec {
  uint32_t* __restrict__ row;  // [cap][kTurnLookRowWords]
  float* __restrict__ value;   // [cap]
};

// The reducing consumer (kernels_turn_lookahead.h): the position and the roll
// the walk starts from in place of an env's, the root forward of that
// position, the replier's side, and the best of the final level's values,
// which the walk leaves here.
struct TurnLook {
  Side s;
  int d0, d1;
  const ValRoot* vr;
  bool smallest;
  float best;
};
__device__ __forceinline__ float turn_look_level(const Side& s, const TurnRoot& r, const uint32_t* pcur, int nrows,
                                                 int level, const ValNet& vn, ValStage& VS, const TurnLook& lk, int lane);

// The picking consumer (kernels_turn_value_rollout.h): the walk starts from
// the position and the roll as the reducing consumer's does (vr is not used:
// the root forward runs behind the walk, once the roll is known to have a
// row); the final level is scored against the position and narde_turn_pick's
// row kept -- its ordinal in the level, white's value of it and, in
// RowBest's payload, its path word -- or, explore, the one row of ordinal
// mulhi(r1, nrows).  level, dh, dl: what turn_path_play needs of the walk.
struct TurnPick : TurnLook {
  bool explore;
  uint32_t r1;
  RowBest b;
  int level, dh, dl;
};
__device__ __forceinline__ void turn_pick_level(const Side& s, const TurnRoot& r, const uint32_t* pcur, int nrows,
                                                int level, const ValNet& vn, ValStage& VS, TurnPick& pk, int lane);

// the position a walk starts from: env e's record, or the reducing consumer's
template <bool kLook>
__device__ __forceinline__ Side turn_position(const TurnArgs& a, int e, const TurnLook* lk) {
  if constexpr (kLook) {
    return lk->s;
  } else {
    return side_from_record(a.pl.p0[e], a.pl.p1[e]);
  }
}

// The level walk of a position under a roll (all lanes of the wave call it
// with the same arguments), and what is done with its final level -- the
// consumers, chosen at compile time.  Returns the number of rows (0: a pass,
// or a die outside 1..6), or -1 if a level outgrew `room` nodes (nothing
// written, nothing reduced).
// key: room + 2 keys of the level being built; pathA, pathB: the two level
// buffers, room paths each.
// The position is env e's record and the roll its dice, or, kLook, lk's (a
// and e are then not looked at).
// kFill: write the rows from row a.offsets[e] on, below a.cap.
// kScore (a fill with a.feat NULL): the rows' values under vn as well
// (kernels_rows.h "the scored rows"; VS the wave's lists).  kRec (a fill
// with a.feat NULL): the rows' records to *tr as well.  kLook (no fill): the
// rows' values under vn against lk->vr reduced to the replier's best, left in
// lk->best.  kPick (with kLook; lk is a TurnPick): the best row and its path
// kept in place of the reduction.  kPub (with kRec): tr->row is the public
// dense output, 8 words a row (kernels_playout_pick.h): the record the step
// leaves and nothing else.
// (The walk and its consumers are one function on purpose, and the existing
// instantiations compile to the instructions they had: with the walk a
// function of its own that hands the final level to its callers -- by
// reference, as a struct, through a callback, or with env e's load in a
// wrapper -- k_turn_overflow_scored ran 2 to 7 % and k_turn_fill_scored up to
// 2 % slower than before, outside the runs' spread; DESIGN.md section 18.2,
// MEASUREMENT_LOG M.34.)
template <bool kFill, bool kScore = false, bool kRec = false, bool kLook = false, bool kPick = false,
          bool kPub = false>
__device__ __forceinline__ int turn_env(const TurnArgs& a, int e, uint64_t* knxt, uint32_t* pathA, uint32_t* pathB,
                                        int room, TurnScan& L, AftStage* S, const ValNet* vn = nullptr,
                                        ValStage* VS = nullptr, const TurnRec* tr = nullptr, TurnLook* lk = nullptr) {
  const int lane = threadIdx.x & 63;
  const Side s = turn_position<kLook>(a, e, lk);
  int d0, d1;
  if constexpr (kLook) {
    d0 = lk->d0;
    d1 = lk->d1;
  } else {
    if (!play_dice(s, a.g, e, a.dice, d0, d1)) return 0;  // wave-uniform
  }
  const TurnRoot r = turn_root(s, d0, d1);
  const bool two = r.dh != r.dl;
  uint32_t* pcur = pathA;
  uint32_t* pnxt = pathB;
  if (lane == 0) pcur[0] = kTurnNoPath;
  wave_lds_handoff();
  int ncur = 1, level = 0, nh1 = 0;
  for (; level < r.depth; ++level) {
    int nnext = 0;
    for (int p0 = 0; p0 < ncur; p0 += 64) {
      {
        const bool act = p0 + lane < ncur;
        const uint32_t path = act ? pcur[p0 + lane] : kTurnNoPath;
        Side c = s;
        turn_path_apply(c, path, act ? level : 0, r.dh, r.dl);
        uint32_t w0, w1;
        turn_node_lists(c, path, level, r, w0, w1);
        w0 = act ? w0 : 0u;
        w1 = act ? w1 : 0u;
        // (wave_scan_incl, and below the earlier-lane key loop and the row
        // stores, written out: through kernels_rows.h's helpers
        // k_turn_overflow measured 1 % slower, MEASUREMENT_LOG M.27)
        int inc = __builtin_popcount(w0 & MASK24) + __builtin_popcount(w1 & MASK24);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int v = __shfl_up(inc, o, 64);
          inc += lane >= o ? v : 0;
        }
        L.incl[lane] = (uint32_t)inc;
        L.w0[lane] = w0;
        L.w1[lane] = w1;
      }
      wave_lds_handoff();
      const int total = __builtin_amdgcn_readfirstlane((int)L.incl[63]);  // <= 64 x 48; scalar: uniform loops
      if (level == 0) nh1 = __builtin_amdgcn_readfirstlane(__builtin_popcount(L.w0[0] & MASK24));
      for (int c0 = 0; c0 < total; c0 += 64) {
        const bool act = c0 + lane < total;
        const int j = act ? c0 + lane : 0;
        // the parent of child j: the first whose inclusive sum exceeds j
        const int pi = wave_owner_of(L.incl, j);
        const int excl = pi ? (int)L.incl[pi - 1] : 0;
        const uint32_t cp = turn_child(pcur[p0 + pi], level, L.w0[pi], L.w1[pi], j - excl);
        const uint64_t key = act ? turn_path_key(cp, level + 1, r.dh, r.dl, two && level == 0) : kTurnNoKey;
        bool dupe = false;
        const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(knxt);
#pragma unroll 4
        for (int q = 0; 2 * q < nnext; ++q) {
          const ulonglong2 v = k2[q];
          dupe |= v.x == key || v.y == key;
        }
        const int nact = min(64, total - c0);
        const int klo = (int)(uint32_t)key, khi = (int)(uint32_t)(key >> 32);
        for (int q = 0; q + 1 < nact; ++q) {
          const uint32_t qlo = (uint32_t)__builtin_amdgcn_readlane(klo, q);
          const uint32_t qhi = (uint32_t)__builtin_amdgcn_readlane(khi, q);
          dupe |= q < lane && qlo == (uint32_t)klo && qhi == (uint32_t)khi;
        }
        const bool keep = act && !dupe;
        int nnew;
        const int rank = wave_keep_rank(keep, lane, nnew);
        if (nnext + nnew > room) return -1;  // wave-uniform: the level does not fit
        if (keep) {
          knxt[nnext + rank] = key;
          pnxt[nnext + rank] = cp;
        }
        if (lane < 2) knxt[nnext + nnew + lane] = kTurnNoKey;
        nnext += nnew;
        wave_lds_handoff();  // the keys, to the next chunk
      }
      wave_lds_handoff();  // the parents' lists are rewritten by the next chunk of parents
    }
    if (nnext == 0) break;
    uint32_t* const pt = pcur;
    pcur = pnxt;
    pnxt = pt;
    ncur = nnext;
  }
  if (level == 0) return 0;  // a pass
  // two different dice and only one playable: the higher die's moves (they
  // come first) if it has any
  const int nrows = (two && level == 1 && nh1 > 0) ? nh1 : ncur;
  if constexpr (kFill) {
    const int64_t row0 = (int64_t)a.offsets[e];
    ValRoot vr;
    if constexpr (kScore) {
      if (row0 >= a.cap) return nrows;  // wave-uniform: every row is past cap
      val_root(vr, *vn, *VS, a.pl.p0[e], a.pl.p1[e], lane);
    }
    for (int g0 = 0; g0 < nrows; g0 += 64) {
      if (row0 + g0 >= a.cap) break;  // wave-uniform: the rest is past cap
      const bool act = g0 + lane < nrows;
      const int64_t R = row0 + g0 + lane;
      const uint32_t path = act ? pcur[g0 + lane] : kTurnNoPath;
      Side c = s;
      turn_path_apply(c, path, act ? level : 0, r.dh, r.dl);
      int term, rew;
      step_end(c, false, term, rew);
      if (a.feat) {
        uint4 ra, rb;
        side_to_record(c, ra, rb);
        S->rec[lane][0] = ra;
        S->rec[lane][1] = rb;
      }
      if constexpr (kScore) {
        if (act) {
          uint4 ra, rb;
          side_to_record(c, ra, rb);
          val_stage_row(*vn, *VS, vr, lane, R, a.cap, ra, rb, rew);
        }
      }
      if (act && R < a.cap) {
        if (a.play) reinterpret_cast<uint64_t*>(a.play)[R] = turn_path_play(path, level, r.dh, r.dl);
        if (a.reward) a.reward[R] = (int8_t)rew;
        if (a.row_env) a.row_env[R] = e;
        if (a.obs) store_obs(a.obs, (size_t)R, c);
        if constexpr (kRec) {
          uint4 ra, rb;
          side_to_record(c, ra, rb);
          if constexpr (kPub) {
            record_close_step(rb);
            uint4* const row = reinterpret_cast<uint4*>(tr->row + R * 8);
            row[0] = ra;
            row[1] = rb;
          } else {
            rb.w = (uint32_t)rew;
            uint4* const row = reinterpret_cast<uint4*>(tr->row + R * kTurnLookRowWords);
            row[0] = ra;
            row[1] = rb;
            tr->row[R * kTurnLookRowWords + kTurnLookRedo] = 0u;
            if (rew != 0) tr->value[R] = val_outcome(rew, (rb.z >> 10) & 1u, 1);
          }
        }
      }
      if (a.feat) aft_flush_feat(a.feat, a.cap, row0 + g0, min(64, nrows - g0), *S, lane);
      if constexpr (kScore) val_score_rows(*vn, *VS, vr, a.cap, row0 + g0, min(64, nrows - g0), lane);
    }
  }
  if constexpr (kLook && !kPick) lk->best = turn_look_level(s, r, pcur, nrows, level, *vn, *VS, *lk, lane);
  if constexpr (kPick) turn_pick_level(s, r, pcur, nrows, level, *vn, *VS, *static_cast<TurnPick*>(lk), lane);
  return nrows;
}

__global__ void __launch_bounds__(kTurnCountBlock) k_turn_count(TurnArgs a) {
  __shared__ TurnFrontLds front[kTurnCountBlock / 64];
  __shared__ TurnScan scan[kTurnCountBlock / 64];
  const int e = aft_wave_env(kTurnCountBlock / 64);
  if (e >= a.n) return;
  TurnFrontLds& F = front[threadIdx.x >> 6];
  const int cnt = turn_env<false>(a, e, F.key, F.path[0], F.path[1], kTurnFront, scan[threadIdx.x >> 6], nullptr);
  if ((threadIdx.x & 63) == 0) {
    a.offsets[e + 1] = cnt < 0 ? 0 : cnt;
    if (cnt < 0) a.ovf[1 + atomicAdd(a.ovf, 1)] = e;  // (at most n appends: every env once)
  }
}

__global__ void __launch_bounds__(kTurnFillBlock) k_turn_fill(TurnArgs a) {
  __shared__ TurnFrontLds front[kTurnFillBlock / 64];
  __shared__ TurnScan scan[kTurnFillBlock / 64];
  __shared__ AftStage stage[kTurnFillBlock / 64];
  const int e = aft_wave_env(kTurnFillBlock / 64);
  if (e >= a.n) return;
  TurnFrontLds& F = front[threadIdx.x >> 6];
  // an env the count pass sent to the overflow list leaves here as it did
  // there, before it writes anything
  turn_env<true>(a, e, F.key, F.path[0], F.path[1], kTurnFront, scan[threadIdx.x >> 6], &stage[threadIdx.x >> 6]);
}

// k_turn_fill with the rows' values in place of their 198 floats (a.feat NULL)
__global__ void __launch_bounds__(kTurnFillBlock) k_turn_fill_scored(TurnArgs a, ValNet vn) {
  __shared__ TurnFrontLds front[kTurnFillBlock / 64];
  __shared__ TurnScan scan[kTurnFillBlock / 64];
  __shared__ ValStage stage[kTurnFillBlock / 64];
  const int e = aft_wave_env(kTurnFillBlock / 64);
  if (e >= a.n) return;
  TurnFrontLds& F = front[threadIdx.x >> 6];
  turn_env<true, true>(a, e, F.key, F.path[0], F.path[1], kTurnFront, scan[threadIdx.x >> 6], nullptr, &vn,
                       &stage[threadIdx.x >> 6]);
}

// The overflow list's envs, a wave each, grid-stride.  First with a
// frontier of kTurnFrontBig nodes a level in the workgroup's LDS (one wave:
// 32.8 KiB), which holds all but the rarest turns; an env that outgrows that
// too is redone with the frontier in the wave's piece of the slab (global
// memory; the wavefront-scope fences of wave_lds_handoff order its
// cross-lane hand-overs as they do LDS's).
constexpr int kTurnFrontBig = 2048;
struct alignas(16) TurnFrontBig {
  uint64_t key[kTurnFrontBig + 2];
  uint32_t path[2][kTurnFrontBig];
};

template <bool kFill>
__global__ void __launch_bounds__(64) k_turn_overflow(TurnArgs a) {
  __shared__ TurnScan scan;
  __shared__ AftStage stage;
  __shared__ TurnFrontBig big;
  uint8_t* const base = a.slab + (size_t)blockIdx.x * kTurnSlabWave;
  uint64_t* const key = reinterpret_cast<uint64_t*>(base);
  uint32_t* const pathA = reinterpret_cast<uint32_t*>(key + kTurnSlabKeys);
  uint32_t* const pathB = pathA + kTurnAftMax;
  const int m = min(a.ovf[0], a.n);
  for (int i = (int)blockIdx.x; i < m; i += (int)gridDim.x) {
    const int e = __builtin_amdgcn_readfirstlane(a.ovf[1 + i]);
    if ((unsigned)e >= (unsigned)a.n) continue;
    int cnt = turn_env<kFill>(a, e, big.key, big.path[0], big.path[1], kTurnFrontBig, scan, &stage);
    if (cnt < 0) {  // wave-uniform
      wave_lds_handoff();
      cnt = turn_env<kFill>(a, e, key, pathA, pathB, kTurnAftMax, scan, &stage);
    }
    // (kTurnAftMax bounds every level: cnt < 0 cannot happen; the test is the bounds guard)
    if (!kFill && (threadIdx.x & 63) == 0) a.offsets[e + 1] = cnt < 0 ? 0 : cnt;
    wave_lds_handoff();
  }
}

// k_turn_overflow<true> with the rows' values in place of their 198 floats
__global__ void __launch_bounds__(64) k_turn_overflow_scored(TurnArgs a, ValNet vn) {
  __shared__ TurnScan scan;
  __shared__ ValStage stage;
  __shared__ TurnFrontBig big;
  uint8_t* const base = a.slab + (size_t)blockIdx.x * kTurnSlabWave;
  uint64_t* const key = reinterpret_cast<uint64_t*>(base);
  uint32_t* const pathA = reinterpret_cast<uint32_t*>(key + kTurnSlabKeys);
  uint32_t* const pathB = pathA + kTurnAftMax;
  const int m = min(a.ovf[0], a.n);
  for (int i = (int)blockIdx.x; i < m; i += (int)gridDim.x) {
    const int e = __builtin_amdgcn_readfirstlane(a.ovf[1 + i]);
    if ((unsigned)e >= (unsigned)a.n) continue;
    int cnt = turn_env<true, true>(a, e, big.key, big.path[0], big.path[1], kTurnFrontBig, scan, nullptr, &vn, &stage);
    if (cnt < 0) {  // wave-uniform
      wave_lds_handoff();
      turn_env<true, true>(a, e, key, pathA, pathB, kTurnAftMax, scan, nullptr, &vn, &stage);
    }
    wave_lds_handoff();
  }
}

}  // namespace
