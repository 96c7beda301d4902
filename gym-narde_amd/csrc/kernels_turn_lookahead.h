// kernels_turn_lookahead.h -- FULL4 two-ply lookahead over whole-turn afterstates
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_turn_afterstates.h and kernels_lookahead.h: the level walk,
// the record fill's TurnRec and look_better are there); not a standalone
// header.
#pragma once

namespace {

// narde_turn_afterstates_lookahead is the count passes and the scan of
// narde_turn_afterstates, then:
//   k_turn_fill_rec, k_turn_overflow_rec
//                   the fills with each kept row's 128-B piece of the call's
//                   scratch written in place of features or a value: the
//                   record the turn leaves (32 B, the ply-counter word = the
//                   reward), the word of rolls to redo cleared; a terminal
//                   row's outcome goes straight to value;
//   k_turn_look     a wave per row -- or, in a short launch, kTurnLookSplit
//                   waves, wave w taking rolls w, w + 4, ...  The row's
//                   record is the root of every reply (val_root, once a
//                   wave).  Per unordered roll a <= b of the opponent
//                   (turn_root orders the dice: (a, b) and (b, a) are one
//                   reply set) the level walk runs on the record with
//                   kTurnFront nodes a level in LDS; its final level is
//                   carried out 64 nodes at a time, staged and scored
//                   against the root (val_stage_row, val_rows_each) and
//                   reduced to the replier's best, which goes to the row's
//                   slot of that roll; a pass scores the record with the
//                   mover flipped (step_end).  A roll whose walk outgrows the
//                   frontier sets its bit in the row's redo word and writes
//                   no slot;
//   k_turn_look_overflow
//                   a fixed grid (kTurnOvfWaves one-wave workgroups) over the
//                   rows' redo words, wave w reading rows w, w + 128, ...,
//                   64 words a load: the marked (row, roll) walks again with
//                   kTurnFrontBig nodes a level in LDS and, past that, in the
//                   wave's piece of the handle's slab -- exact for every
//                   position;
//   k_turn_look_mean
//                   a lane per row: the weighted mean of the slots (1 a
//                   double, 2 otherwise) in roll order, in double, rounded
//                   once.
// Every (row, roll) best is written by one wave to a slot of its own and the
// mean reads them in a fixed order: no atomics, the same bits on every call,
// for every cap and for either launch shape.
//
// A wave has 10.4 KiB of LDS (frontier 4.0, lists 0.8, scored rows 5.6): 3
// waves a SIMD, 3,072 on the device's 1,024 SIMDs.  Up to that many rows a
// launch of one wave a row leaves SIMDs idle and lasts as long as its slowest
// row; kTurnLookSplit waves a row fill them (the root forward is then paid
// once a wave, which longer launches avoid).
constexpr int kTurnLookSplit = 4;
constexpr int64_t kTurnLookSplitRows = 3072;
constexpr int kTurnLookRolls = 21;
constexpr int kTurnLookMeanBlock = 256;
static_assert(kTurnLookBest + kTurnLookRolls <= kTurnLookRedo && kTurnLookRedo < kTurnLookRowWords,
              "a row's piece holds the record, the rolls' bests and the redo word");
static_assert(NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES(1) == 4 * kTurnLookRowWords, "narde.h states the same row piece");

struct TurnLookArgs {
  uint32_t* __restrict__ row;           // [cap][kTurnLookRowWords], the record fills'
  const int32_t* __restrict__ offsets;  // [n + 1]
  int n;
  int64_t cap;
  int dice_mode;
  uint8_t* __restrict__ slab;           // [kTurnOvfWaves][kTurnSlabWave]
};

__global__ void __launch_bounds__(kTurnFillBlock) k_turn_fill_rec(TurnArgs a, TurnRec tr) {
  __shared__ TurnFrontLds front[kTurnFillBlock / 64];
  __shared__ TurnScan scan[kTurnFillBlock / 64];
  const int e = aft_wave_env(kTurnFillBlock / 64);
  if (e >= a.n) return;
  TurnFrontLds& F = front[threadIdx.x >> 6];
  turn_env<true, false, true>(a, e, F.key, F.path[0], F.path[1], kTurnFront, scan[threadIdx.x >> 6], nullptr, nullptr,
                              nullptr, &tr);
}

// k_turn_overflow<true> with the rows' records in place of their 198 floats
__global__ void __launch_bounds__(64) k_turn_overflow_rec(TurnArgs a, TurnRec tr) {
  __shared__ TurnScan scan;
  __shared__ TurnFrontBig big;
  uint8_t* const base = a.slab + (size_t)blockIdx.x * kTurnSlabWave;
  uint64_t* const key = reinterpret_cast<uint64_t*>(base);
  uint32_t* const pathA = reinterpret_cast<uint32_t*>(key + kTurnSlabKeys);
  uint32_t* const pathB = pathA + kTurnAftMax;
  const int m = min(a.ovf[0], a.n);
  for (int i = (int)blockIdx.x; i < m; i += (int)gridDim.x) {
    const int e = __builtin_amdgcn_readfirstlane(a.ovf[1 + i]);
    if ((unsigned)e >= (unsigned)a.n) continue;
    int cnt = turn_env<true, false, true>(a, e, big.key, big.path[0], big.path[1], kTurnFrontBig, scan, nullptr,
                                          nullptr, nullptr, &tr);
    if (cnt < 0) {  // wave-uniform
      wave_lds_handoff();
      turn_env<true, false, true>(a, e, key, pathA, pathB, kTurnAftMax, scan, nullptr, nullptr, nullptr, &tr);
    }
    wave_lds_handoff();
  }
}

// the replier's best of white's values over the final level a walk of s
// under r left (nrows > 0 nodes of `level` sub-moves in pcur): 64 nodes at a
// time carried out, staged against the root and scored, a min / max in place
// of a store, six shuffle steps.  All lanes of the wave call it with the same
// arguments and get the same float.
__device__ __forceinline__ float turn_look_level(const Side& s, const TurnRoot& r, const uint32_t* pcur, int nrows,
                                                 int level, const ValNet& vn, ValStage& VS, const TurnLook& lk, int lane) {
  const bool smallest = lk.smallest;
  const ValRoot& vr = *lk.vr;
  float best = smallest ? __builtin_inff() : -__builtin_inff();
  for (int g0 = 0; g0 < nrows; g0 += 64) {
    const bool act = g0 + lane < nrows;
    const uint32_t path = act ? pcur[g0 + lane] : kTurnNoPath;
    Side c = s;
    turn_path_apply(c, path, act ? level : 0, r.dh, r.dl);
    int term, rew;
    step_end(c, false, term, rew);
    if (act) {
      uint4 ca, cb;
      side_to_record(c, ca, cb);
      val_stage_row(vn, VS, vr, lane, 0, 0, ca, cb, rew);  // (cap 0: nothing is stored)
      if (rew != 0) best = look_better(best, val_outcome(rew, (cb.z >> 10) & 1u, 1), smallest);
    }
    val_rows_each(vn, VS, vr, min(64, nrows - g0), [&](int, float v) { best = look_better(best, v, smallest); });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = look_better(best, __shfl_xor(best, o, 64), smallest);
  return best;
}

// a pass: the value of what the step with an all -1 play leaves -- s with
// the mover flipped, one staged row (all lanes, the same float)
__device__ __forceinline__ float turn_look_pass(const Side& s, const ValNet& vn, ValStage& VS, const ValRoot& vr,
                                                int lane) {
  Side c = s;
  int term, rew;
  step_end(c, false, term, rew);
  uint4 ca, cb;
  side_to_record(c, ca, cb);
  float best = 0.0f;
  if (lane == 0) {
    val_stage_row(vn, VS, vr, 0, 0, 0, ca, cb, rew);
    if (rew != 0) best = val_outcome(rew, (cb.z >> 10) & 1u, 1);
  }
  val_rows_each(vn, VS, vr, 1, [&](int, float v) { best = v; });
  return __shfl(best, 0, 64);
}

// the (row, roll) walk of lk's position under (d0, d1) with `room` nodes a
// level: the replier's best in `best`; returns false if a level outgrew room
__device__ __forceinline__ bool turn_look_roll(TurnLook& lk, int d0, int d1, uint64_t* knxt, uint32_t* pathA,
                                               uint32_t* pathB, int room, TurnScan& L, const ValNet& vn, ValStage& VS,
                                               int lane, float& best) {
  const TurnArgs none{};
  lk.d0 = d0;
  lk.d1 = d1;
  const int nrows = turn_env<false, false, false, true>(none, 0, knxt, pathA, pathB, room, L, nullptr, &vn, &VS, nullptr,
                                                        &lk);
  if (nrows < 0) return false;
  best = nrows == 0 ? turn_look_pass(lk.s, vn, VS, *lk.vr, lane) : lk.best;
  return true;
}

// launched over cap rows: a workgroup whose row is at or past
// min(offsets[n], cap) leaves, and so does a terminal row's (its value is the
// fill's, its redo word 0)
// (a row per workgroup of kWaves waves: every exit before the barrier is the whole workgroup's)
// kGiven (narde_turn_records_lookahead), here and in the
// two passes below: the rows are the n pieces k_turn_look_pack made of the
// caller's records -- rows = n, no offsets; a finished record's piece has word
// 7 set, as a terminal row's.  New instantiations: the existing ones are the
// ones they were.
template <bool kGiven>
__device__ __forceinline__ int64_t turn_look_rows(const TurnLookArgs& a) {
  if constexpr (kGiven) return (int64_t)a.n;
  else return min((int64_t)a.offsets[a.n], a.cap);
}

template <int kWaves, bool kGiven = false>
__global__ void __launch_bounds__(64 * kWaves) k_turn_look(TurnLookArgs a, ValNet vn) {
  __shared__ TurnFrontLds front[kWaves];
  __shared__ TurnScan scan[kWaves];
  __shared__ ValStage stage[kWaves];
  __shared__ uint32_t wave_redo[kWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  TurnFrontLds& F = front[wave];
  TurnScan& L = scan[wave];
  ValStage& VS = stage[wave];
  const int lane = threadIdx.x & 63;
  const int64_t R = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const int64_t rows = turn_look_rows<kGiven>(a);
  if (R >= rows) return;
  uint32_t* const row = a.row + R * kTurnLookRowWords;
  const uint4 ra = reinterpret_cast<const uint4*>(row)[0];
  const uint4 rb = reinterpret_cast<const uint4*>(row)[1];
  if (rb.w != 0u) return;  // the turn's reward: a terminal row
  const Side s = side_from_record(ra, rb);
  ValRoot vr;
  val_root(vr, vn, VS, ra, rb, lane);
  TurnLook lk{s, 0, 0, &vr, s.black != 0u, 0.0f};  // the values are white's: black replies with the smallest
  uint32_t redo = 0u;
  int k = 0;
  for (int d0 = 1; d0 <= 6; ++d0) {
    for (int d1 = d0; d1 <= 6; ++d1, ++k) {
      if (a.dice_mode == NARDE_DICE_NODOUBLES && d0 == d1) continue;
      if (kWaves > 1 && k % kWaves != wave) continue;  // wave-uniform
      wave_lds_handoff();  // the last roll's reads of the frontier are done
      float best;
      if (!turn_look_roll(lk, d0, d1, F.key, F.path[0], F.path[1], kTurnFront, L, vn, VS, lane, best)) {
        redo |= 1u << k;  // wave-uniform: the overflow pass's
        continue;
      }
      if (lane == 0) reinterpret_cast<float*>(row)[kTurnLookBest + k] = best;
    }
  }
  if constexpr (kWaves == 1) {
    if (lane == 0) row[kTurnLookRedo] = redo;
  } else {
    if (lane == 0) wave_redo[wave] = redo;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) all |= wave_redo[w];
      row[kTurnLookRedo] = all;
    }
  }
}

// The marked (row, roll) walks again, exact for every position.  Wave w
// reads the redo words of rows w, w + 128, ..., lane = row (consecutive rows
// -- one env's -- go to different waves); a marked row's root forward runs
// once, then each marked roll's walk with kTurnFrontBig nodes a level in LDS
// and, if that is outgrown too, in the wave's piece of the slab.
template <bool kGiven = false>
__global__ void __launch_bounds__(64) k_turn_look_overflow(TurnLookArgs a, ValNet vn) {
  __shared__ TurnScan scan;
  __shared__ ValStage stage;
  __shared__ TurnFrontBig big;
  uint8_t* const base = a.slab + (size_t)blockIdx.x * kTurnSlabWave;
  uint64_t* const key = reinterpret_cast<uint64_t*>(base);
  uint32_t* const pathA = reinterpret_cast<uint32_t*>(key + kTurnSlabKeys);
  uint32_t* const pathB = pathA + kTurnAftMax;
  const int lane = threadIdx.x & 63;
  const int64_t rows = turn_look_rows<kGiven>(a);
  const int64_t waves = (int64_t)gridDim.x;
  for (int64_t i0 = 0; (i0 * waves + (int64_t)blockIdx.x) < rows; i0 += 64) {
    const int64_t Rl = (i0 + lane) * waves + (int64_t)blockIdx.x;
    uint32_t mine = 0u;
    if (Rl < rows && a.row[Rl * kTurnLookRowWords + 7] == 0u) mine = a.row[Rl * kTurnLookRowWords + kTurnLookRedo];
    uint64_t marked = __ballot(mine != 0u);
    while (marked) {  // wave-uniform
      const int q = __builtin_ctzll(marked);
      marked &= marked - 1ull;
      const int64_t R = (i0 + q) * waves + (int64_t)blockIdx.x;
      uint32_t redo = (uint32_t)__builtin_amdgcn_readlane((int)mine, q) & ((1u << kTurnLookRolls) - 1u);
      uint32_t* const row = a.row + R * kTurnLookRowWords;
      const uint4 ra = reinterpret_cast<const uint4*>(row)[0];
      const uint4 rb = reinterpret_cast<const uint4*>(row)[1];
      const Side s = side_from_record(ra, rb);
      ValRoot vr;
      val_root(vr, vn, stage, ra, rb, lane);
      TurnLook lk{s, 0, 0, &vr, s.black != 0u, 0.0f};
      int k = 0;
      for (int d0 = 1; d0 <= 6; ++d0) {
        for (int d1 = d0; d1 <= 6; ++d1, ++k) {
          if (!((redo >> k) & 1u)) continue;  // wave-uniform
          wave_lds_handoff();
          float best;
          bool fits = turn_look_roll(lk, d0, d1, big.key, big.path[0], big.path[1], kTurnFrontBig, scan, vn, stage, lane,
                                     best);
          if (!fits) {  // wave-uniform
            wave_lds_handoff();
            fits = turn_look_roll(lk, d0, d1, key, pathA, pathB, kTurnAftMax, scan, vn, stage, lane, best);
          }
          if (!fits) continue;  // (kTurnAftMax bounds every level: cannot happen; the bounds guard)
          if (lane == 0) reinterpret_cast<float*>(row)[kTurnLookBest + k] = best;
        }
      }
      wave_lds_handoff();
    }
  }
}

// value[R] = sum w m / sum w over the dice mode's unordered rolls a <= b, a
// outer, b inner, w = 1 for a double and 2 otherwise; in double, rounded once
template <bool kGiven = false>
__global__ void __launch_bounds__(kTurnLookMeanBlock) k_turn_look_mean(TurnLookArgs a, float* __restrict__ value) {
  const int64_t R = (int64_t)blockIdx.x * kTurnLookMeanBlock + threadIdx.x;
  const int64_t rows = turn_look_rows<kGiven>(a);
  if (R >= rows) return;
  const uint32_t* const row = a.row + R * kTurnLookRowWords;
  if (row[7] != 0u) return;  // a terminal row: the fill's outcome stands (kGiven: the pack's NaN)
  const float* const best = reinterpret_cast<const float*>(row) + kTurnLookBest;
  double sum = 0.0, weight = 0.0;
  int k = 0;
  for (int d0 = 1; d0 <= 6; ++d0) {
    for (int d1 = d0; d1 <= 6; ++d1, ++k) {
      if (a.dice_mode == NARDE_DICE_NODOUBLES && d0 == d1) continue;
      const double w = d0 == d1 ? 1.0 : 2.0;
      sum += w * (double)best[k];
      weight += w;
    }
  }
  value[R] = (float)(sum / weight);
}

// narde_turn_records_lookahead's first pass, a lane per record: the caller's
// public record into its 128-B row piece, as the record fills leave one -- word
// 7 (the caller's ply counter, which no pass may read as a reward) replaced by
// the mark of a finished record (record_finished), whose value is NaN here and
// which the passes above then leave alone as a terminal row; the redo word
// cleared.  The caller's records are only read.
__global__ void __launch_bounds__(kTurnLookMeanBlock) k_turn_look_pack(const uint4* __restrict__ records, int64_t n,
                                                                       uint32_t* __restrict__ row,
                                                                       float* __restrict__ value) {
  const int64_t R = (int64_t)blockIdx.x * kTurnLookMeanBlock + threadIdx.x;
  if (R >= n) return;
  const uint4 ra = records[2 * R];
  uint4 rb = records[2 * R + 1];
  const bool done = record_finished(rb.z);
  rb.w = done ? 1u : 0u;
  uint32_t* const piece = row + R * kTurnLookRowWords;
  reinterpret_cast<uint4*>(piece)[0] = ra;
  reinterpret_cast<uint4*>(piece)[1] = rb;
  piece[kTurnLookRedo] = 0u;
  if (done) value[R] = __builtin_nanf("");
}

}  // namespace
