// kernels_rows.h -- what an afterstate row set is, for both rule sets (DESIGN.md sections 13 and 14)
// Part of the one translation unit narde.hip (included there, in order);
// not a standalone header.
#pragma once

namespace {

// Both expansions (REF2's plays, FULL4's whole turns) give CSR rows: a count
// pass leaves env e's row count in offsets[e + 1], k_aft_scan turns the
// counts into offsets, a fill pass writes env e's rows from offsets[e] on,
// below cap -- the narrow outputs (aft_store_row, and the kind's own action
// column) from the row's lane, the 198 floats through LDS (aft_flush_feat)
// or, in the scored fills, the row's value under a small MLP in their place
// (val_score_rows).  k_aft_pick chooses a row per env by value.  A wave
// works on one env.

// ------------------------------------------------------------ wave helpers
__device__ __forceinline__ int wave_scan_incl(int x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    x += lane >= o ? y : 0;
  }
  return x;
}

// the owner of item j among 64 inclusive sums (LDS): the first that exceeds j
__device__ __forceinline__ int wave_owner_of(const uint32_t* incl, int j) {
  int i = 0;
#pragma unroll
  for (int st = 32; st > 0; st >>= 1) i += (int)incl[i + st - 1] <= j ? st : 0;
  return i;
}

// the lane's rank among the kept lanes (those below it) and their number:
// kept items take their places in lane order with no atomics
__device__ __forceinline__ int wave_keep_rank(bool keep, int lane, int& nkeep) {
  const uint64_t bal = __ballot(keep);
  const int rank = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
  nkeep = __builtin_popcountll(bal);
  return rank;
}

// an earlier lane of this chunk (nact active lanes) holds the same key
// (v_readlane: the loop is wave-uniform).  32-bit keys only: turn_env writes
// its 64-bit loop out, as it does wave_scan_incl and aft_store_row -- through
// these helpers k_turn_overflow ran 1 % slower (MEASUREMENT_LOG M.27).
__device__ __forceinline__ bool wave_key_in_earlier_lane(uint32_t key, int lane, int nact) {
  bool dupe = false;
  for (int q = 0; q + 1 < nact; ++q) {
    const uint32_t kq = (uint32_t)__builtin_amdgcn_readlane((int)key, q);
    dupe |= q < lane && kq == key;
  }
  return dupe;
}

// the wave's env index as a scalar: the record and dice loads and every
// branch on them are wave-uniform
__device__ __forceinline__ int aft_wave_env(int waves) {
  return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves + (threadIdx.x >> 6)));
}

// ------------------------------------------------------------ the rows
constexpr int kAftRows = 8;  // feature rows staged per flush

struct alignas(16) AftStage {  // per wave, fill pass
  uint4 rec[64][2];                // the chunk's kept afterstate records, by rank
  float rows[kAftRows * 198 + 4];  // the staged rows, 8 B in at an odd first row
};

// row R's narrow outputs, from the row's lane (R < cap; the kind's action
// column is the caller's)
__device__ __forceinline__ void aft_store_row(int32_t* __restrict__ row_env, int8_t* __restrict__ reward,
                                              int32_t* __restrict__ obs, int64_t R, int e, int rew, const Side& c) {
  if (reward) reward[R] = (int8_t)rew;
  if (row_env) row_env[R] = e;
  if (obs) store_obs(obs, (size_t)R, c);
}

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

// ------------------------------------------------------------ the scored rows
// aft_flush_feat's sibling: instead of a row's 198
// floats, its value under a 198 -> H -> 1 MLP -- one float.  The env's own
// pre-activations are computed once (val_root); a row's are those plus its
// few differing columns' weight rows (narde_rules.h val_row_list: the row's
// lane lists them in LDS).  The rows are then scored kValRows at a time, 16
// lanes a row, lane t of a row holding hidden units t, t + 16, ...: reads of
// W1t rows through the cache (64 B a lane group and unit), the activation,
// w2, a sum over the 16 lanes and one store.  The kernels are bound by the
// number of instructions, not by memory: this layout keeps every lane busy
// for any H, and a row costs about a quarter of what one row a wave did
// (MEASUREMENT_LOG M.30).
static_assert(kValHiddenMax == NARDE_VALUE_HIDDEN_MAX, "narde.h and narde_rules.h state the same bound");

struct ValNet {
  const float* __restrict__ w1t;  // [198][ld]
  int64_t ld;
  const float* __restrict__ b1;   // [hidden]
  const float* __restrict__ w2;   // [hidden]
  const float* __restrict__ b2;   // [1]
  int hidden, hidden_act, out_act, perspective;
  float* __restrict__ value;      // [cap]
};

struct alignas(16) ValStage {  // per wave, scored fill pass
  uint2 list[64][kValRowSlots];  // the chunk's rows' column lists, by rank
  uint2 root[kValRootSlots];     // the env's own columns
  int cnt[64];                   // a row's list length; -1: a terminal row, its outcome is written
};

struct ValRoot {  // per lane: the env's record and pre-activations, the lane's weights
  uint4 ra, rb;
  float z[kValUnits], w2[kValUnits], b2;
  int t, g, nu;
};

// the env's part of the scoring, once per env (all lanes, the same record)
__device__ __forceinline__ void val_root(ValRoot& r, const ValNet& n, ValStage& S, const uint4& ra, const uint4& rb,
                                         int lane) {
  r.ra = ra;
  r.rb = rb;
  r.t = lane & (kValLanes - 1);
  r.g = lane / kValLanes;
  r.nu = (n.hidden + kValLanes - 1) / kValLanes;
#pragma unroll
  for (int i = 0; i < kValUnits; ++i) r.z[i] = r.w2[i] = 0.0f;  // (units past nu are never read)
  wave_lds_handoff();  // (earlier reads of S.root are done)
  {  // the record's columns: lane = item, the items' entries placed by a prefix sum
    int col[4];
    float val[4];
    const int c = tes_item_nonzero(ra, rb, lane, col, val);
    const int incl = wave_scan_incl(c, lane);
    const int total = min(__builtin_amdgcn_readlane(incl, 63), kValRootSlots);  // 33 at most; the bounds guard
    const int npad = (total + kValRootBatch - 1) / kValRootBatch * kValRootBatch;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < c && incl - c + j < kValRootSlots) S.root[incl - c + j] = val_entry(col[j], val[j], n.ld);
    if (total + lane < npad) S.root[total + lane] = make_uint2(0u, 0u);
    wave_lds_handoff();
    val_units(r.nu, [&](auto NU) {
      val_root_part<NU.value>(S.root, npad, r.g, n.w1t, r.t, n.hidden, r.z);
#pragma unroll
      for (int i = 0; i < NU.value; ++i) {
        const bool on = r.t + kValLanes * i < n.hidden;
        // ((p0 + p1) + (p2 + p3)) + b1, the same bits in every lane group
        const float pair = r.z[i] + __shfl_xor(r.z[i], kValLanes, 64);
        r.z[i] = (pair + __shfl_xor(pair, 2 * kValLanes, 64)) + (on ? n.b1[r.t + kValLanes * i] : 0.0f);
        r.w2[i] = on ? n.w2[r.t + kValLanes * i] : 0.0f;  // (0 past hidden: such a unit adds nothing)
      }
    });
  }
  r.b2 = n.b2[0];
}

// row R's (rank `rank` of its chunk) part, from the row's lane: its column
// list staged -- a terminal row's empty, its outcome written (R < cap)
__device__ __forceinline__ void val_stage_row(const ValNet& n, ValStage& S, const ValRoot& r, int rank, int64_t R,
                                              int64_t cap, const uint4& ca, const uint4& cb, int rew) {
  if (rew != 0) {
    S.cnt[rank] = -1;
    for (int k = 0; k < kValRowSlots; ++k) S.list[rank][k] = make_uint2(0u, 0u);
    if (R < cap) n.value[R] = val_outcome(rew, (cb.z >> 10) & 1u, n.perspective);
  } else {
    S.cnt[rank] = val_row_list(r.ra, r.rb, ca, cb, n.ld, S.list[rank]);
  }
}

// the values of the first nr rows a chunk staged, kValRows rows at a time (a
// short batch repeats the last row): out(q, v) from lane 0 of the lane group
// that scored staged row q, terminal rows left out.  All lanes of the wave
// call it with the same arguments.
template <typename F>
__device__ __forceinline__ void val_rows_each(const ValNet& n, ValStage& S, const ValRoot& r, int nr, F&& out) {
  wave_lds_handoff();  // the lists, to every lane
  val_units(r.nu, [&](auto NU) {
    for (int q0 = 0; q0 < nr; q0 += kValRows) {
      const int q = min(q0 + r.g, nr - 1);
      const int cnt = S.cnt[q];
      if (__ballot(cnt >= 0) == 0ull) continue;  // wave-uniform: terminal rows only
      const bool more = __ballot(cnt > kValRowFirst) != 0ull;
      float z[kValUnits];
#pragma unroll
      for (int i = 0; i < NU.value; ++i) z[i] = r.z[i];
      val_row_z<NU.value>(S.list[q], more, n.w1t, r.t, n.hidden, z);
      float part = val_lane_part<NU.value>(z, r.w2, n.hidden_act);
#pragma unroll
      for (int o = kValLanes / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      if (r.t == 0 && q0 + r.g < nr && cnt >= 0) out(q, val_out_act(r.b2 + part, n.out_act));
    }
  });
  wave_lds_handoff();  // the next chunk's lists are staged behind these reads
}

// the values of the nnew rows a chunk staged -> value rows Rbase .. Rbase +
// nnew - 1, below cap.  All lanes of the wave call it with the same arguments.
__device__ __forceinline__ void val_score_rows(const ValNet& n, ValStage& S, const ValRoot& r, int64_t cap,
                                               int64_t Rbase, int nnew, int lane) {
  const int64_t room = cap - Rbase;
  const int nr = room < (int64_t)nnew ? (int)room : nnew;  // wave-uniform: the rest is past cap
  val_rows_each(n, S, r, nr, [&](int q, float v) { n.value[Rbase + q] = v; });
}

// ------------------------------------------------------------ counts -> offsets
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

// ------------------------------------------------------------ the pick
// One row per env from value[r * ld]: the largest (perspective 0: the
// values are the mover's; perspective 1: they are white's, README.md:42-102,
// and white moves) or the smallest (perspective 1 and black moves), the
// lowest row on ties, a NaN taken as torch.max / torch.min(dim) take it (the
// first NaN).  Rows from cap on do not exist.  With epsilon, the env's
// explore draw Philox4x32-10({*tag, env, 0, 5}, seed) r0 < epsilon * 2^32
// (the policy kernels' decision) takes row offsets[e] + mulhi(r1, count)
// instead.  An env with no row: -1.
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

// The row by aft_pick_row and its entry of the action column, one word W a
// row -- REF2: the two int16 codes, kNoRow 0 = actions (0, 0); FULL4: the
// (4,2) int8 play, kNoRow -1 = every byte -1.  One lane per env.
template <typename W, int kNoRow>
__global__ void __launch_bounds__(kBlock) k_aft_pick(Planes pl, int n, const int32_t* __restrict__ offsets,
                                                     const W* __restrict__ column, int64_t cap,
                                                     const float* __restrict__ value, int64_t ld, int perspective,
                                                     const float* __restrict__ eps_p,
                                                     const int64_t* __restrict__ tag_p, uint32_t k0, uint32_t k1,
                                                     W* __restrict__ out, int32_t* __restrict__ row_out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t row = aft_pick_row(pl, i, offsets, cap, value, ld, perspective, eps_p, tag_p, k0, k1);
  out[i] = row >= 0 ? column[row] : static_cast<W>(kNoRow);
  if (row_out) row_out[i] = (int32_t)row;
}

}  // namespace
