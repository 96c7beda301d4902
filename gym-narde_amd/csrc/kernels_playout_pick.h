// kernels_playout_pick.h -- playout-greedy play: the rows' records, an env's top-K rows, the pick over playouts
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_turn_lookahead.h: aft_env, turn_env and the overflow
// launches' frontier are there); not a standalone header.
#pragma once

namespace {

// ------------------------------------------------------------ the rows' records
// narde_afterstates_records / narde_turn_afterstates_records: the fills of the
// scored expansions (or, with no net, of the plain ones less their features)
// with each kept row's record written as a dense 32-B row of the caller's --
// the kRec path of aft_env / turn_env in its public form (kPub): the record
// the step that plays the row leaves, its ply counter included.  New
// instantiations: the existing fills are the ones they were.
__global__ void __launch_bounds__(kAftFillBlock) k_aft_fill_records(AftArgs a, AftRec ar) {
  __shared__ AftScan scan[kAftFillBlock / 64];
  const int e = aft_wave_env(kAftFillBlock / 64);
  if (e >= a.n) return;
  aft_env<true, false, true, true>(a, e, scan[threadIdx.x >> 6], nullptr, nullptr, nullptr, &ar);
}

__global__ void __launch_bounds__(kAftFillBlock) k_aft_fill_scored_records(AftArgs a, ValNet vn, AftRec ar) {
  __shared__ AftScan scan[kAftFillBlock / 64];
  __shared__ ValStage stage[kAftFillBlock / 64];
  const int e = aft_wave_env(kAftFillBlock / 64);
  if (e >= a.n) return;
  aft_env<true, true, true, true>(a, e, scan[threadIdx.x >> 6], nullptr, &vn, &stage[threadIdx.x >> 6], &ar);
}

// FULL4: k_turn_fill / k_turn_fill_scored and the overflow launches, the same way
template <bool kScore>
__global__ void __launch_bounds__(kTurnFillBlock) k_turn_fill_records(TurnArgs a, ValNet vn, TurnRec tr) {
  __shared__ TurnFrontLds front[kTurnFillBlock / 64];
  __shared__ TurnScan scan[kTurnFillBlock / 64];
  __shared__ ValStage stage[kTurnFillBlock / 64];
  const int e = aft_wave_env(kTurnFillBlock / 64);
  if (e >= a.n) return;
  TurnFrontLds& F = front[threadIdx.x >> 6];
  turn_env<true, kScore, true, false, false, true>(a, e, F.key, F.path[0], F.path[1], kTurnFront,
                                                   scan[threadIdx.x >> 6], nullptr, &vn, &stage[threadIdx.x >> 6], &tr);
}

template <bool kScore>
__global__ void __launch_bounds__(64) k_turn_overflow_records(TurnArgs a, ValNet vn, TurnRec tr) {
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
    int cnt = turn_env<true, kScore, true, false, false, true>(a, e, big.key, big.path[0], big.path[1], kTurnFrontBig,
                                                               scan, nullptr, &vn, &stage, &tr);
    if (cnt < 0) {  // wave-uniform
      wave_lds_handoff();
      turn_env<true, kScore, true, false, false, true>(a, e, key, pathA, pathB, kTurnAftMax, scan, nullptr, &vn, &stage,
                                                       &tr);
    }
    wave_lds_handoff();
  }
}

// ------------------------------------------------------------ top-K rows per env
// narde_rows_topk: a wave per env, k rounds of the pick's reduction.  A round
// offers a row only if the round before's choice is strictly ahead of it in
// argmax_takes' total order (topk_offers), so no list of the chosen is kept;
// a lane takes rows lane, lane + 64, ..., and six shuffle steps merge the
// lanes' bests -- a total order: every lane ends with the same row, and the
// same bits on every call.  Lanes 0 and 1 copy the row's record to the root.
constexpr int kTopkBlock = 256;  // 4 envs per workgroup

struct TopkArgs {
  Planes pl;
  int n;
  const int32_t* __restrict__ offsets;  // [n + 1]
  int64_t cap;
  const float* __restrict__ value;  // [cap] x ld
  int64_t ld;
  int perspective, k;
  const uint4* __restrict__ records;  // [cap][2] or NULL
  int32_t* __restrict__ sel;          // [n][k]
  uint4* __restrict__ roots;          // [n][k][2] or NULL
};

__global__ void __launch_bounds__(kTopkBlock) k_rows_topk(TopkArgs a) {
  const int e = aft_wave_env(kTopkBlock / 64);
  if (e >= a.n) return;
  const int lane = threadIdx.x & 63;
  const int64_t r0 = a.offsets[e];
  const int64_t r1 = min((int64_t)a.offsets[e + 1], a.cap);
  const int cnt = r1 > r0 ? (int)(r1 - r0) : 0;
  const bool smallest = a.perspective == 1 && ((a.pl.p1[e].z >> 10) & 1u);
  float px = 0.0f;
  int pi = -1;
  for (int i = 0; i < a.k; ++i) {
    float bx = 0.0f;
    int bi = -1;
    if (i < cnt) {  // wave-uniform: a row is left
      for (int q = lane; q < cnt; q += 64) {
        const float v = a.value[(r0 + q) * a.ld];
        const float x = smallest ? -v : v;  // as aft_pick_row
        if (topk_offers(px, pi, x, q) && argmax_takes(x, q, bx, bi)) { bx = x; bi = q; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ox = __shfl_xor(bx, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (argmax_takes(ox, oi, bx, bi)) { bx = ox; bi = oi; }
      }
    }
    px = bx;
    pi = bi;
    const int64_t row = bi >= 0 ? r0 + bi : -1;
    const size_t slot = (size_t)e * (size_t)a.k + (size_t)i;
    if (lane == 0) a.sel[slot] = (int32_t)row;
    if (a.roots && lane < 2)
      a.roots[2 * slot + lane] = row >= 0 ? a.records[2 * row + lane]
                                          : make_uint4(0u, 0u, lane ? kRecordNoneWord6 : 0u, 0u);
  }
}

// ------------------------------------------------------------ the pick over the playouts' sums
// narde_playout_pick / narde_turn_playout_pick: a lane per env walks its k
// slots (playout_pick_slot: integer sums, the leaves added in trial order in
// double, one division, one rounding) and writes the chosen row's entry of the
// action column as k_aft_pick does -- one word W a row, kNoRow for an env
// with no candidate.  The values are white's: the mover is the env's record's.
struct PlayoutPickArgs {
  Planes pl;
  int n, k, trials;
  const int32_t* __restrict__ sel;    // [n][k]
  int64_t cap;
  const float* __restrict__ value;    // [cap] x ld
  int64_t ld;
  const int8_t* __restrict__ reward;  // [cap]
  const int32_t* __restrict__ sums;   // [n * k][4]
  const float* __restrict__ leaf;     // [n * k][trials] or NULL
  int32_t* __restrict__ row;          // [n] or NULL
  float* __restrict__ score;          // [n][k] or NULL
};

template <typename W, int kNoRow>
__global__ void __launch_bounds__(kBlock) k_playout_pick(PlayoutPickArgs a, const W* __restrict__ column,
                                                         W* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const size_t s0 = (size_t)i * (size_t)a.k;
  const bool smallest = ((a.pl.p1[i].z >> 10) & 1u) != 0u;
  const int bi = playout_pick_slot(a.sel + s0, a.k, a.cap, a.value, a.ld, a.reward, a.sums + 4 * s0,
                                   a.leaf ? a.leaf + s0 * (size_t)a.trials : nullptr, a.trials, smallest,
                                   a.score ? a.score + s0 : nullptr);
  const int64_t r = bi >= 0 ? (int64_t)a.sel[s0 + bi] : -1;
  out[i] = r >= 0 ? column[r] : static_cast<W>(kNoRow);
  if (a.row) a.row[i] = (int32_t)r;
}

// ------------------------------------------------------------ the pick over given slot scores
// narde_slot_pick / narde_turn_slot_pick: k_playout_pick
// with the caller's score a slot in place of the playouts' sums
// (slot_pick_slot); the same outputs.
struct SlotPickArgs {
  Planes pl;
  int n, k;
  const int32_t* __restrict__ sel;    // [n][k]
  int64_t cap;
  const float* __restrict__ value;    // [cap] x ld
  int64_t ld;
  const int8_t* __restrict__ reward;  // [cap]
  const float* slot_score;            // [n][k]
  int32_t* __restrict__ row;          // [n] or NULL
  float* score;                       // [n][k] or NULL (may be slot_score itself)
};

template <typename W, int kNoRow>
__global__ void __launch_bounds__(kBlock) k_slot_pick(SlotPickArgs a, const W* __restrict__ column,
                                                      W* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const size_t s0 = (size_t)i * (size_t)a.k;
  const bool smallest = ((a.pl.p1[i].z >> 10) & 1u) != 0u;
  const int bi = slot_pick_slot(a.sel + s0, a.k, a.cap, a.value, a.ld, a.reward, a.slot_score + s0, smallest,
                                a.score ? a.score + s0 : nullptr);
  const int64_t r = bi >= 0 ? (int64_t)a.sel[s0 + bi] : -1;
  out[i] = r >= 0 ? column[r] : static_cast<W>(kNoRow);
  if (a.row) a.row[i] = (int32_t)r;
}

}  // namespace
