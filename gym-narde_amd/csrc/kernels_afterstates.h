// kernels_afterstates.h -- REF2 afterstate expansion: the play enumeration
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_rows.h: the row set, the scan, the pick and the wave
// helpers are there); not a standalone header.
#pragma once

namespace {

// A wave per env (narde_rules.h "afterstates" gives the semantics):
//   1. lanes 0..47 hold the 48 possible list-#1 entries (lane = 24 k + p:
//      k = 0 the higher die's list, source p) and compute their kPlayStep
//      words in parallel (play_step_word: apply_move + die_filter); a wave
//      prefix sum of their play counts gives every entry its play range;
//   2. the plays go 64 per chunk, one per lane: the lane finds its entry in
//      the prefix sums (6-step search in LDS), builds its play, the
//      expressible flag and the 20-bit dedupe key (play_key), and compares the
//      key with the kept plays of earlier chunks (LDS, four keys a read) and
//      with the earlier lanes of its own chunk (v_readlane);
//   3. a ballot of the survivors and a popcount below the lane give each its
//      row: rows are in enumeration order with no atomics.
// aft_entries is step 1, aft_chunks steps 2 and 3; the position is an env's
// record here and a row's in the lookahead pass (kernels_lookahead.h).
// The count pass stops there (the env's count -> offsets[e + 1], then
// k_aft_scan); the fill pass also builds each survivor's afterstate, writes
// its narrow outputs from the lane, and stages the 198-float rows 8 at a
// time in LDS (tes_stage_quarter, as k_tesauro198_rows) to stream them out
// as the env's contiguous byte run.
constexpr int kAftMaxPlays = 48 * 24;  // structural bound: 48 entries x 24 second-move sources
constexpr int kAftCountBlock = 256;    // count pass: 4 envs per workgroup
constexpr int kAftFillBlock = 64;      // fill pass: an env per workgroup (13.2 KiB of LDS a wave: 3 waves per SIMD)
constexpr uint32_t kAftNoKey = 0xFFFFFFFFu;

struct AftArgs {
  Planes pl;
  int n;
  Rng g;
  const uint8_t* __restrict__ dice;
  int64_t cap;
  int32_t* __restrict__ offsets;  // [n + 1]
  int32_t* __restrict__ row_env;  // [cap]
  int16_t* __restrict__ codes;    // [cap][2]
  float* __restrict__ feat;       // [cap][198]
  int32_t* __restrict__ obs;      // [cap][24]
  int8_t* __restrict__ reward;    // [cap]
};

struct alignas(16) AftScan {  // per wave, both passes
  uint32_t keys[kAftMaxPlays + 4];  // kept plays' keys, kAftNoKey behind the last (four a read)
  uint32_t incl[64];                // inclusive prefix sums of the entries' play counts
  uint32_t word[64];                // the entries' kPlayStep words
};

// Step 1 for the position s and the roll (d0, d1), l = legal2(s, d0, d1): the
// entries' words and the prefix sums of their play counts into L; returns
// the number of plays (scalar).  All lanes of the wave call it with the same
// position: an env's record (aft_env) or a row's (kernels_lookahead.h).
__device__ __forceinline__ int aft_entries(const Side& s, int d0, int d1, const Legal& l, AftScan& L, int lane) {
  const int n1 = l.count;
  {
    const int k = lane >= 24 ? 1 : 0, p = (lane - 24 * k) & 31;
    const uint32_t Lk = k ? l.L[1] : l.L[0];
    uint32_t word = 0u;
    int plays = 0;
    if (lane < 48 && ((Lk >> p) & 1u)) {
      word = play_step_word(s, d0, d1, n1, p, k ? l.d[1] : l.d[0]);
      plays = play_step_count(n1, word, play_entry_dup(l, k, p));
    }
    L.incl[lane] = (uint32_t)wave_scan_incl(plays, lane);
    L.word[lane] = word;
  }
  wave_lds_handoff();
  return __builtin_amdgcn_readfirstlane((int)L.incl[63]);  // <= kAftMaxPlays; scalar: uniform loops
}

// Steps 2 and 3 over the `total` plays aft_entries left in L, 64 a chunk:
// chunk(nkept, keep, rank, nnew, y) once per chunk, by every lane -- nkept
// rows kept before the chunk, the lane's play y kept or not, its rank among
// the chunk's nnew kept.  Returns the number of rows.
template <typename F>
__device__ __forceinline__ int aft_chunks(const Legal& l, int total, AftScan& L, int lane, F&& chunk) {
  const int n1 = l.count;
  int nkept = 0;
  for (int c0 = 0; c0 < total; c0 += 64) {
    const bool act = c0 + lane < total;
    const int j = act ? c0 + lane : 0;
    // the entry of play j: the first whose inclusive sum exceeds j
    const int ei = wave_owner_of(L.incl, j);
    const int ek = ei >= 24 ? 1 : 0;
    const int excl = ei ? (int)L.incl[ei - 1] : 0;
    const Play y = play_of_entry(ei - 24 * ek, ek ? l.d[1] : l.d[0], L.word[ei], j - excl);
    const bool expr = act && play_expressible(y, n1 == 1);
    const uint32_t key = expr ? play_key(y) : kAftNoKey;
    bool dupe = false;
    const uint4* k4 = reinterpret_cast<const uint4*>(L.keys);
    for (int q = 0; 4 * q < nkept; ++q) {
      const uint4 v = k4[q];
      dupe |= v.x == key || v.y == key || v.z == key || v.w == key;
    }
    dupe |= wave_key_in_earlier_lane(key, lane, min(64, total - c0));
    const bool keep = expr && !dupe;
    int nnew;
    const int rank = wave_keep_rank(keep, lane, nnew);
    if (keep) L.keys[nkept + rank] = key;
    if (lane < 3) L.keys[nkept + nnew + lane] = kAftNoKey;
    chunk(nkept, keep, rank, nnew, y);
    nkept += nnew;
    wave_lds_handoff();  // the keys, to the next chunk
  }
  return nkept;
}

// What the record fill (kernels_lookahead.h) writes besides the narrow
// outputs: row R's record after the step at rec[2 R], rec[2 R + 1] -- its
// ply-counter word replaced by the step's reward, which the lookahead pass
// reads as "terminal" -- and a terminal row's outcome in white's perspective.
struct AftRec {
  uint4* __restrict__ rec;    // [cap][2]
  float* __restrict__ value;  // [cap]
};

// env e's rows (all lanes of the wave call it with the same e); returns the
// number of rows.  kFill: write them from row a.offsets[e] on, below a.cap.
// kScore (a fill with a.feat NULL): the rows' values under vn as well
// (kernels_rows.h "the scored rows"; VS the wave's lists).  kRec (a fill
// with a.feat NULL): the rows' records to *ar as well -- kPub: in the public
// form (kernels_playout_pick.h), the record the step leaves and nothing else.
template <bool kFill, bool kScore = false, bool kRec = false, bool kPub = false>
__device__ __forceinline__ int aft_env(const AftArgs& a, int e, AftScan& L, AftStage* S, const ValNet* vn = nullptr,
                                       ValStage* VS = nullptr, const AftRec* ar = nullptr) {
  const int lane = threadIdx.x & 63;
  const Side s = side_from_record(a.pl.p0[e], a.pl.p1[e]);
  int d0, d1;
  if (!play_dice(s, a.g, e, a.dice, d0, d1)) return 0;  // wave-uniform
  Legal l;
  legal2(s, d0, d1, l);
  const int total = aft_entries(s, d0, d1, l, L, lane);
  const int64_t row0 = kFill ? (int64_t)a.offsets[e] : 0;
  ValRoot vr;
  if constexpr (kScore) {
    if (total == 0) return 0;  // wave-uniform: no play, nothing to score
    val_root(vr, *vn, *VS, a.pl.p0[e], a.pl.p1[e], lane);
  }
  return aft_chunks(l, total, L, lane, [&](int nkept, bool keep, int rank, int nnew, const Play& y) {
    if constexpr (kFill) {
      const int64_t R = row0 + nkept + rank;
      if (keep) {
        Side c = s;
        int term, rew;
        play_afterstate(c, y, term, rew);
        if (a.feat) {
          uint4 ra, rb;
          side_to_record(c, ra, rb);
          S->rec[rank][0] = ra;
          S->rec[rank][1] = rb;
        }
        if constexpr (kScore) {
          uint4 ra, rb;
          side_to_record(c, ra, rb);
          val_stage_row(*vn, *VS, vr, rank, R, a.cap, ra, rb, rew);
        }
        if (R < a.cap) {
          int c1, c2;
          play_codes(y, c1, c2);
          if (a.codes)
            reinterpret_cast<uint32_t*>(a.codes)[R] = (uint32_t)(uint16_t)c1 | ((uint32_t)(uint16_t)c2 << 16);
          aft_store_row(a.row_env, a.reward, a.obs, R, e, rew, c);
          if constexpr (kRec) {
            uint4 ra, rb;
            side_to_record(c, ra, rb);
            if constexpr (kPub) {
              record_close_step(rb);
              ar->rec[2 * R] = ra;
              ar->rec[2 * R + 1] = rb;
            } else {
              rb.w = (uint32_t)rew;
              ar->rec[2 * R] = ra;
              ar->rec[2 * R + 1] = rb;
              if (rew != 0) ar->value[R] = val_outcome(rew, (rb.z >> 10) & 1u, 1);
            }
          }
        }
      }
      if (a.feat) aft_flush_feat(a.feat, a.cap, row0 + nkept, nnew, *S, lane);
      if constexpr (kScore) val_score_rows(*vn, *VS, vr, a.cap, row0 + nkept, nnew, lane);
    }
  });
}

__global__ void __launch_bounds__(kAftCountBlock) k_aft_count(AftArgs a) {
  __shared__ AftScan scan[kAftCountBlock / 64];
  const int e = aft_wave_env(kAftCountBlock / 64);
  if (e >= a.n) return;
  const int cnt = aft_env<false>(a, e, scan[threadIdx.x >> 6], nullptr);
  if ((threadIdx.x & 63) == 0) a.offsets[e + 1] = cnt;
}

__global__ void __launch_bounds__(kAftFillBlock) k_aft_fill(AftArgs a) {
  __shared__ AftScan scan[kAftFillBlock / 64];
  __shared__ AftStage stage[kAftFillBlock / 64];
  const int e = aft_wave_env(kAftFillBlock / 64);
  if (e >= a.n) return;
  aft_env<true>(a, e, scan[threadIdx.x >> 6], &stage[threadIdx.x >> 6]);
}

// k_aft_fill with the rows' values in place of their 198 floats (a.feat NULL)
__global__ void __launch_bounds__(kAftFillBlock) k_aft_fill_scored(AftArgs a, ValNet vn) {
  __shared__ AftScan scan[kAftFillBlock / 64];
  __shared__ ValStage stage[kAftFillBlock / 64];
  const int e = aft_wave_env(kAftFillBlock / 64);
  if (e >= a.n) return;
  aft_env<true, true>(a, e, scan[threadIdx.x >> 6], nullptr, &vn, &stage[threadIdx.x >> 6]);
}

}  // namespace

