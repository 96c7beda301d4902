// kernels_td_window.h -- windowed TD(lambda) on the value MLP
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_td.h: TdNet, TdStage, td_forward and k_td_update are there);
// not a standalone header.
#pragma once

namespace {

// narde_value_td_window: the forward view of TD(lambda) over a recorded window
// of K plies, the weights held fixed over it -- theta += alpha sum G_k grad
// v(s_k) --, with no trace array: a sample's gradient has its record's own
// ~25 columns and the tail, and goes from td_forward's LDS pieces straight
// into an accumulator on chip.
//   k_tdw_values   a wave a sample, (K + 1) B of them: v(s_k) by
//                  td_forward<false> on the stored record (s_K: the env's own);
//   k_tdw_returns  a thread an env: delta_k and G_k backward over k;
//   k_tdw_grad     a workgroup a slab of kTdwSlab consecutive samples: the
//                  dense accumulator of P = 200 H + 1 floats in dynamic LDS,
//                  one partial row a slab;
//   k_td_update    (kernels_td.h) the partial rows in slab order, into the
//                  weights and the mirror.
// No float atomics: every accumulator element has one owner thread, which
// takes the samples in order.
constexpr int kTdwWaves = kTdBlock / 64;
static_assert(kTdwSlab == NARDE_TD_WINDOW_SLAB, "narde.h and narde_rules.h state the same slab");
static_assert(kTdwSlab % kTdwWaves == 0, "whole batches of samples");
static_assert(kValHiddenMax * 2 <= kTdBlock, "k_tdw_grad: two column classes at least");

// sample i's record: a stored one below K B, the env's own behind them
__device__ __forceinline__ void tdw_record(const uint4* __restrict__ records, const Planes& pl, int64_t stored,
                                           int64_t i, uint4& ra, uint4& rb) {
  if (i < stored) {  // wave-uniform
    ra = records[2 * i];
    rb = records[2 * i + 1];
  } else {
    ra = pl.p0[i - stored];
    rb = pl.p1[i - stored];
  }
}

__global__ void __launch_bounds__(kTdBlock) k_tdw_values(Planes pl, const uint4* __restrict__ records, int64_t stored,
                                                         int64_t samples, TdNet net, float* __restrict__ v) {
  __shared__ TdStage S[kTdwWaves];
  const int64_t i = (int64_t)blockIdx.x * kTdwWaves + (int64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= samples) return;  // wave-uniform
  uint4 ra, rb;
  tdw_record(records, pl, stored, i, ra, rb);
  const float val = td_forward<false>(net, S[threadIdx.x >> 6], ra, rb, (int)(threadIdx.x & 63));
  if ((threadIdx.x & 63) == 0) v[i] = val;
}

// env e, k = K - 1 .. 0: delta_k from v_k and v_{k+1}, G_k from G_{k+1}
__global__ void __launch_bounds__(kTdBlock) k_tdw_returns(int n, int plies, const uint32_t* __restrict__ records,
                                                          const float* __restrict__ v,
                                                          const int32_t* __restrict__ reward,
                                                          const uint8_t* __restrict__ terminated,
                                                          const uint8_t* __restrict__ truncated, float gamma, float gl,
                                                          float* __restrict__ G, float* __restrict__ delta) {
  const int e = (int)(blockIdx.x * kTdBlock + threadIdx.x);
  if (e >= n) return;
  float vn = v[(int64_t)plies * n + e], gn = 0.0f;
  for (int k = plies - 1; k >= 0; --k) {
    const int64_t i = (int64_t)k * n + e;
    const float vk = v[i];
    const bool tm = terminated[i] != 0, tr = truncated[i] != 0;
    const uint32_t black = (records[8 * i + 6] >> 10) & 1u;  // the record's misc word
    const float d = td_delta(tm, tr, reward[i], black, gamma, vn, vk);
    gn = td_return(d, tm || tr, gl, gn);
    if (delta) delta[i] = d;
    G[i] = gn;
    vn = vk;
  }
}

// what the accumulating threads need of a sample beside its TdStage: the
// listed columns (val_root_list's order, then b1's and w2's), each with the
// column class that owns it, and the sample's G
struct alignas(16) TdwList {
  uint32_t ent[kValRootSlots + 2];  // column | class << 8
  int n;
  float G;
};

// grid: the slabs; 2 kTdBlock threads.  The first kTdBlock threads forward
// the slab's samples, kTdwWaves at a time, a wave each, into one of two sets
// of stages; the other kTdBlock accumulate the set before it, so a batch's
// forward (the latency of its weight reads) runs beside the last batch's
// adds.  Accumulating thread (class g, unit h) = (t / H, t % H), g below
// 256 / H, owns the accumulator elements (c, h) with c % (256 / H) == g: for
// every sample, in sample order, it walks the sample's list and adds where
// the column is its own.
__global__ void __launch_bounds__(2 * kTdBlock) k_tdw_grad(const uint4* __restrict__ records, int64_t samples,
                                                           TdNet net, const float* __restrict__ G,
                                                           float* __restrict__ part, int64_t ld_part) {
  extern __shared__ float4 tdw_lds[];
  float* const acc = reinterpret_cast<float*>(tdw_lds);
  __shared__ TdStage S[2][kTdwWaves];
  __shared__ TdwList W[2][kTdwWaves];
  const int H = net.hidden;
  const int P = kTdCols * H + 1;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool forwards = wave < kTdwWaves;  // wave-uniform
  const int classes = kTdBlock / H;        // 2 at least
  const int t = tid - kTdBlock, g = t / H, h = t - g * H;  // (the accumulating threads')
  const int64_t i0 = (int64_t)blockIdx.x * kTdwSlab;
  const int ns = (int)min((int64_t)kTdwSlab, samples - i0);
  const int nbatch = (ns + kTdwWaves - 1) / kTdwWaves;
  for (int p = tid; p < P; p += 2 * kTdBlock) acc[p] = 0.0f;
  for (int b = 0; b <= nbatch; ++b) {
    __syncthreads();  // the zeroes; batch b - 1 is staged, batch b - 2 is added
    if (forwards) {
      const int j = b * kTdwWaves + wave;
      if (j < ns) {  // wave-uniform
        const int64_t i = i0 + j;
        const uint4 ra = records[2 * i], rb = records[2 * i + 1];
        TdwList& L = W[b & 1][wave];
        td_forward<true>(net, S[b & 1][wave], ra, rb, lane);
        // the columns by slot, as td_forward placed their values in S.cols.xv
        int col[4];
        float val[4];
        const int c = tes_item_nonzero(ra, rb, lane, col, val);
        const int incl = wave_scan_incl(c, lane);
        const int total = min(__builtin_amdgcn_readlane(incl, 63), kValRootSlots);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = incl - c + q;
          if (q < c && k < kValRootSlots) L.ent[k] = (uint32_t)col[q] | ((uint32_t)(col[q] % classes) << 8);
        }
        if (lane < 2) L.ent[total + lane] = (uint32_t)(kTdColB1 + lane) | ((uint32_t)((kTdColB1 + lane) % classes) << 8);
        if (lane == 0) {
          L.n = total + 2;
          L.G = G[i];
        }
      }
    } else if (b > 0 && g < classes) {
      const int nb = min(kTdwWaves, ns - (b - 1) * kTdwWaves);
      for (int w = 0; w < nb; ++w) {
        const TdStage& T = S[(b - 1) & 1][w];
        const TdwList& L = W[(b - 1) & 1][w];
        const float Gs = L.G, d = T.d[h], ga = T.ga[h];
        const int n = L.n;
        for (int q = 0; q < n; ++q) {
          const uint32_t ent = L.ent[q];
          if ((int)(ent >> 8) == g) {
            const int c = (int)(ent & 255u);
            float* a = acc + c * H + h;
            *a = tdw_acc(*a, Gs, c, c < kTdColB1 ? T.cols.xv[q] : 1.0f, d, ga);
          }
        }
        if (t == 0) acc[P - 1] = tdw_acc_b2(acc[P - 1], Gs, T.go);
      }
    }
  }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * ld_part;
  for (int p = tid; p < P; p += 2 * kTdBlock) out[p] = acc[p];
}

}  // namespace
