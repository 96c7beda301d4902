// kernels_afterstates.h -- batched afterstate expansion and the value-greedy pick
// Part of the one translation unit narde.hip (included there, in order);
// not a standalone header.
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
// The count pass stops there (the env's count -> offsets[e + 1], then
// k_aft_scan); the fill pass also builds each survivor's afterstate, writes
// its narrow outputs from the lane, and stages the 198-float rows 8 at a
// time in LDS (tes_stage_quarter, as k_tesauro198_rows) to stream them out
// as the env's contiguous byte run.
constexpr int kAftMaxPlays = 48 * 24;  // structural bound: 48 entries x 24 second-move sources
constexpr int kAftRows = 8;            // feature rows staged per flush
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

struct alignas(16) AftStage {  // per wave, fill pass
  uint4 rec[64][2];                // the chunk's kept afterstate records, by rank
  float rows[kAftRows * 198 + 4];  // the staged rows, 8 B in at an odd first row
};

// The 198-float rows of the nnew records a chunk left in S.rec (by rank) ->
// feat rows R0 .. R0 + nnew - 1, below cap: staged kAftRows at a time
// (tes_stage_quarter) and streamed out as one contiguous byte run.  All
// lanes of the wave call it with the same arguments.
__device__ __forceinline__ void aft_flush_feat(float* __restrict__ feat, int64_t cap, int64_t Rbase, int nnew,
                                               AftStage& S, int lane) {
  wave_lds_handoff();  // the records, to the lanes that stage them
  for (int g0 = 0; g0 < nnew; g0 += kAftRows) {
    const int64_t R0 = Rbase + g0;
    const int64_t room = cap - R0;
    const int want = min(kAftRows, nnew - g0);
    const int nr = room < (int64_t)want ? (int)room : want;
    if (nr <= 0) break;  // wave-uniform: the rest is past cap
    // a row is 792 B: an odd first row starts 8 B into a 16-B piece, and
    // so do the staged rows, so every piece is aligned on both sides
    const int ph = (int)(R0 & 1) * 2;
    const int le = lane & 15;  // (kAftRows of the 16 row slots of tes_stage_rows' lane layout)
    if (le < nr) tes_stage_quarter(S.rec[g0 + le][0], S.rec[g0 + le][1], lane >> 4, S.rows + ph + le * 198);
    wave_lds_handoff();
    const uint32_t lo = 4u * (uint32_t)ph, hi = lo + (uint32_t)nr * kTesRowB;
    const float4* src = reinterpret_cast<const float4*>(S.rows);
    float4* dst = reinterpret_cast<float4*>(feat + R0 * 198 - ph);
    for (uint32_t k = (uint32_t)lane; 16u * k < hi; k += 64u) {
      const uint32_t b0 = 16u * k;
      if (b0 >= lo && b0 + 16u <= hi) {
        dst[k] = src[k];
      } else {  // the run starts or ends inside this piece: its 8-B half
        const int h = b0 < lo ? 2 : 0;
        *reinterpret_cast<float2*>(reinterpret_cast<float*>(dst + k) + h) =
            *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(src + k) + h);
      }
    }
    wave_lds_handoff();  // the next rows are staged behind these reads
  }
}

// env e's rows (all lanes of the wave call it with the same e); returns the
// number of rows.  kFill: write them from row a.offsets[e] on, below a.cap.
template <bool kFill>
__device__ __forceinline__ int aft_env(const AftArgs& a, int e, AftScan& L, AftStage* S) {
  const int lane = threadIdx.x & 63;
  const Side s = side_from_record(a.pl.p0[e], a.pl.p1[e]);
  int d0, d1;
  if (!play_dice(s, a.g, e, a.dice, d0, d1)) return 0;  // wave-uniform
  Legal l;
  legal2(s, d0, d1, l);
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
    int inc = plays;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      inc += lane >= o ? v : 0;
    }
    L.incl[lane] = (uint32_t)inc;
    L.word[lane] = word;
  }
  wave_lds_handoff();
  const int total = __builtin_amdgcn_readfirstlane((int)L.incl[63]);  // <= kAftMaxPlays; scalar: uniform loops
  const int64_t row0 = kFill ? (int64_t)a.offsets[e] : 0;
  int nkept = 0;
  for (int c0 = 0; c0 < total; c0 += 64) {
    const bool act = c0 + lane < total;
    const int j = act ? c0 + lane : 0;
    // the entry of play j: the first whose inclusive sum exceeds j
    int ei = 0;
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) ei += (int)L.incl[ei + st - 1] <= j ? st : 0;
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
    const int nact = min(64, total - c0);
    for (int q = 0; q + 1 < nact; ++q) {
      const uint32_t kq = (uint32_t)__builtin_amdgcn_readlane((int)key, q);
      dupe |= q < lane && kq == key;
    }
    const bool keep = expr && !dupe;
    const uint64_t bal = __ballot(keep);
    const int rank = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    const int nnew = __builtin_popcountll(bal);
    if (keep) L.keys[nkept + rank] = key;
    if (lane < 3) L.keys[nkept + nnew + lane] = kAftNoKey;
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
        if (R < a.cap) {
          int c1, c2;
          play_codes(y, c1, c2);
          if (a.codes)
            reinterpret_cast<uint32_t*>(a.codes)[R] = (uint32_t)(uint16_t)c1 | ((uint32_t)(uint16_t)c2 << 16);
          if (a.reward) a.reward[R] = (int8_t)rew;
          if (a.row_env) a.row_env[R] = e;
          if (a.obs) store_obs(a.obs, (size_t)R, c);
        }
      }
      if (a.feat) aft_flush_feat(a.feat, a.cap, row0 + nkept, nnew, *S, lane);
    }
    nkept += nnew;
    wave_lds_handoff();  // the keys, to the next chunk
  }
  return nkept;
}

// the wave's env index as a scalar: the record and dice loads and every
// branch on them are wave-uniform
__device__ __forceinline__ int aft_wave_env(int waves) {
  return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves + (threadIdx.x >> 6)));
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

// offsets[1..n] (the count pass's per-env counts) -> their inclusive sums,
// offsets[0] = 0.  One workgroup; a tile is 32 rows of 1,024 counts, count
// k * 1024 + t with thread t, so every load and store of a wave is one
// contiguous 256 B (32 consecutive counts a thread left one CU's address
// path 64 lines per instruction: 60 us at B = 65,536).  Every row is scanned
// inside its waves, the 32 x 16 wave totals -- in index order as laid out --
// are scanned by wave 0, and the running total is carried from tile to tile.
constexpr int kAftScanBlock = 1024;
constexpr int kAftScanItems = 32;
constexpr int kAftScanWaves = kAftScanBlock / 64;

__device__ __forceinline__ int wave_scan_incl(int x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    x += lane >= o ? y : 0;
  }
  return x;
}

__global__ void __launch_bounds__(kAftScanBlock) k_aft_scan(int32_t* __restrict__ offsets, int n) {
  constexpr int kTotals = kAftScanItems * kAftScanWaves;  // 512: 8 a lane of wave 0
  __shared__ int wsum[kTotals];
  __shared__ int tile_total;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kAftScanBlock * kAftScanItems) {
    int v[kAftScanItems];
#pragma unroll
    for (int k = 0; k < kAftScanItems; ++k) {
      const int i = base + k * kAftScanBlock + (int)threadIdx.x;
      v[k] = i < n ? offsets[i + 1] : 0;
    }
#pragma unroll
    for (int k = 0; k < kAftScanItems; ++k) {
      v[k] = wave_scan_incl(v[k], lane);
      if (lane == 63) wsum[k * kAftScanWaves + wave] = v[k];
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the wave totals, in place
      int x[kTotals / 64], sum = 0;
#pragma unroll
      for (int q = 0; q < kTotals / 64; ++q) {
        x[q] = wsum[lane * (kTotals / 64) + q];
        sum += x[q];
      }
      const int inc = wave_scan_incl(sum, lane);
      int run = inc - sum;
#pragma unroll
      for (int q = 0; q < kTotals / 64; ++q) {
        wsum[lane * (kTotals / 64) + q] = run;
        run += x[q];
      }
      if (lane == 63) tile_total = inc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kAftScanItems; ++k) {
      const int i = base + k * kAftScanBlock + (int)threadIdx.x;
      if (i < n) offsets[i + 1] = carry + wsum[k * kAftScanWaves + wave] + v[k];
    }
    carry += tile_total;
    __syncthreads();  // wsum and tile_total are rewritten by the next tile
  }
  if (threadIdx.x == 0) offsets[0] = 0;
}

// One row per env from value[r * ld]: the largest (perspective 0: the
// values are the mover's; perspective 1: they are white's, README.md:42-102,
// and white moves) or the smallest (perspective 1 and black moves), the
// lowest row on ties, a NaN taken as torch.max / torch.min(dim) take it (the
// first NaN).  Rows from cap on do not exist.  With epsilon, the env's
// explore draw Philox4x32-10({*tag, env, 0, 5}, seed) r0 < epsilon * 2^32
// (the policy kernels' decision) takes row offsets[e] + mulhi(r1, count)
// instead.  An env with no row: row -1, actions (0, 0).  One lane per env.
// (aft_pick_row: the selection, shared with k_turn_pick.)
__device__ __forceinline__ int64_t aft_pick_row(const Planes& pl, int i, const int32_t* __restrict__ offsets,
                                                int64_t cap, const float* __restrict__ value, int64_t ld,
                                                int perspective, const float* __restrict__ eps_p,
                                                const int64_t* __restrict__ tag_p, uint32_t k0, uint32_t k1) {
  const int64_t r0 = offsets[i];
  const int64_t r1 = min((int64_t)offsets[i + 1], cap);
  const int cnt = r1 > r0 ? (int)(r1 - r0) : 0;
  int64_t row = -1;
  if (cnt > 0) {
    bool explore = false;
    if (eps_p) {
      uint32_t r[4];
      philox4x32_10((uint32_t)*tag_p, (uint32_t)i, 0u, 5u, k0, k1, r);
      explore = (uint64_t)r[0] < eps_to_q32(*eps_p);
      if (explore) row = r0 + (int64_t)mulhi_u32(r[1], (uint32_t)cnt);
    }
    if (!explore) {
      const bool smallest = perspective == 1 && ((pl.p1[i].z >> 10) & 1u);
      float best = 0.0f;
      int bi = -1;
      for (int q = 0; q < cnt; ++q) {
        const float v = value[(r0 + q) * ld];
        const float x = smallest ? -v : v;  // argmin(v) = argmax(-v), ties and NaNs alike
        if (argmax_takes(x, q, best, bi)) { best = x; bi = q; }
      }
      row = r0 + bi;
    }
  }
  return row;
}

__global__ void __launch_bounds__(kBlock) k_aft_pick(Planes pl, int n, const int32_t* __restrict__ offsets,
                                                     const int16_t* __restrict__ codes, int64_t cap,
                                                     const float* __restrict__ value, int64_t ld, int perspective,
                                                     const float* __restrict__ eps_p,
                                                     const int64_t* __restrict__ tag_p, uint32_t k0, uint32_t k1,
                                                     int16_t* __restrict__ actions, int32_t* __restrict__ row_out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t row = aft_pick_row(pl, i, offsets, cap, value, ld, perspective, eps_p, tag_p, k0, k1);
  const uint32_t pair = row >= 0 ? reinterpret_cast<const uint32_t*>(codes)[row] : 0u;
  reinterpret_cast<uint32_t*>(actions)[i] = pair;
  if (row_out) row_out[i] = (int32_t)row;
}

}  // namespace
