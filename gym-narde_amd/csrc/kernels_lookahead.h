// kernels_lookahead.h -- REF2 two-ply lookahead: the expected best reply per afterstate
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_afterstates.h: the play enumeration, the record fill's
// AftRec and the scored rows' helpers are there); not a standalone header.
#pragma once

namespace {

// narde_afterstates_lookahead is the count pass and the scan of
// narde_afterstates, then two passes of its own:
//   k_aft_fill_rec  the fill with each kept row's record (32 B) written to
//                   the call's scratch in place of features or a value; a
//                   terminal row's outcome goes straight to value;
//   k_aft_look      a wave per row.  The row's record is the root of every
//                   reply (val_root, once): a reply differs from it in at
//                   most 6 columns, as a row does from its env.  Per roll of
//                   the opponent the play enumeration runs on the record
//                   (aft_entries / aft_chunks), the kept replies are staged
//                   and scored as the scored fill does (val_stage_row,
//                   val_rows_each) and reduced to the replier's best in
//                   place of a store; a roll with no reply scores what the
//                   step with the codes (0, 0) leaves (env_step): nearly
//                   always the record with the mover flipped -- the two
//                   player columns.  The
//                   rolls are taken as ordered pairs (a, b), a outer, b
//                   inner, and summed in that order in double: no atomics,
//                   the same bits on every call.
// A wave takes a row's 36 rolls in 0.55 ms, so a launch that does not fill
// the device (B = 64: 867 rows for 1,024 SIMDs) lasts as long as one wave:
// up to kLookSplitRows rows the row's workgroup is kLookSplit waves, wave w
// taking rolls w, w + 4, ..., each roll's best left in LDS and summed by one
// lane in the same order -- the same bits as one wave a row, which longer
// launches keep (the root forward is paid once a wave).
constexpr int kLookSplit = 4;
constexpr int64_t kLookSplitRows = 3072;  // x 4 waves = the device's 1,024 SIMDs x 3 waves (10.7 KiB of LDS a wave)

struct LookArgs {
  const uint4* __restrict__ rec;        // [cap][2], k_aft_fill_rec's
  const int32_t* __restrict__ offsets;  // [n + 1]
  int n;
  int64_t cap;
  int dice_mode;
};

__global__ void __launch_bounds__(kAftFillBlock) k_aft_fill_rec(AftArgs a, AftRec ar) {
  __shared__ AftScan scan[kAftFillBlock / 64];
  const int e = aft_wave_env(kAftFillBlock / 64);
  if (e >= a.n) return;
  aft_env<true, false, true>(a, e, scan[threadIdx.x >> 6], nullptr, nullptr, nullptr, &ar);
}

// the replier's better of two of white's values: black takes the smaller
__device__ __forceinline__ float look_better(float x, float y, bool smallest) {
  return smallest ? fminf(x, y) : fmaxf(x, y);
}

// launched over cap rows: a wave whose row is at or past min(offsets[n], cap)
// leaves, and so does a terminal row's (its value is the fill's)
// (a row per workgroup of kWaves waves: every exit before the barrier is the whole workgroup's)
// kGiven (narde_records_lookahead): the rows are the
// caller's n public records -- rows = n, no offsets; word 7 is the ply counter
// and is not looked at; a finished record (record_finished) gets NaN.  New
// instantiations: the existing two are the ones they were.
template <int kWaves, bool kGiven = false>
__global__ void __launch_bounds__(64 * kWaves) k_aft_look(LookArgs a, ValNet vn) {
  __shared__ AftScan scan[kWaves];
  __shared__ ValStage stage[kWaves];
  __shared__ float roll_best[36];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  AftScan& L = scan[wave];
  ValStage& VS = stage[wave];
  const int lane = threadIdx.x & 63;
  const int64_t R = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  int64_t rows;
  if constexpr (kGiven) rows = a.n;
  else rows = min((int64_t)a.offsets[a.n], a.cap);
  if (R >= rows) return;
  const uint4 ra = a.rec[2 * R];
  const uint4 rb = a.rec[2 * R + 1];
  if constexpr (kGiven) {
    if (record_finished(rb.z)) {  // no two-ply value
      if (threadIdx.x == 0) vn.value[R] = __builtin_nanf("");
      return;
    }
  } else {
    if (rb.w != 0u) return;  // the step's reward: a terminal row
  }
  const Side s = side_from_record(ra, rb);
  const bool smallest = s.black != 0u;  // the values are white's: black replies with the smallest
  ValRoot vr;
  val_root(vr, vn, VS, ra, rb, lane);
  double sum = 0.0;
  int rolls = 0;
  for (int d0 = 1; d0 <= 6; ++d0) {
    for (int d1 = 1; d1 <= 6; ++d1) {
      if (a.dice_mode == NARDE_DICE_NODOUBLES && d0 == d1) continue;
      const int k = rolls++;
      if (kWaves > 1 && k % kWaves != wave) continue;  // wave-uniform
      Legal l;
      legal2(s, d0, d1, l);
      const int total = aft_entries(s, d0, d1, l, L, lane);
      float best = smallest ? __builtin_inff() : -__builtin_inff();
      const int replies = aft_chunks(l, total, L, lane, [&](int, bool keep, int rank, int nnew, const Play& y) {
        if (keep) {
          Side c = s;
          int term, rew;
          play_afterstate(c, y, term, rew);
          uint4 ca, cb;
          side_to_record(c, ca, cb);
          val_stage_row(vn, VS, vr, rank, 0, 0, ca, cb, rew);  // (cap 0: nothing is stored)
          if (rew != 0) best = look_better(best, val_outcome(rew, (cb.z >> 10) & 1u, 1), smallest);
        }
        val_rows_each(vn, VS, vr, nnew, [&](int, float v) { best = look_better(best, v, smallest); });
      });
      if (replies == 0) {  // wave-uniform: what the step with the codes (0, 0) leaves -- a pass, or a
        Side c = s;         // bear-off from point 0 whose plays no code can express
        StepOut o;
        env_step(c, d0, d1, 0, 0, false, 0u, 0u, o);
        uint4 ca, cb;
        side_to_record(c, ca, cb);
        if (lane == 0) {
          val_stage_row(vn, VS, vr, 0, 0, 0, ca, cb, o.reward);
          if (o.reward != 0) best = val_outcome(o.reward, (cb.z >> 10) & 1u, 1);
        }
        val_rows_each(vn, VS, vr, 1, [&](int, float v) { best = v; });
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = look_better(best, __shfl_xor(best, o, 64), smallest);
      if constexpr (kWaves == 1) {
        sum += (double)best;
      } else {
        if (lane == 0) roll_best[k] = best;
      }
    }
  }
  if constexpr (kWaves > 1) {
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 0; k < rolls; ++k) sum += (double)roll_best[k];
  }
  if (threadIdx.x == 0) vn.value[R] = (float)(sum / (double)rolls);
}

}  // namespace
