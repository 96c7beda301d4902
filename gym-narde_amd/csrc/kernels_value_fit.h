// kernels_value_fit.h -- the value MLP's supervised fit and the playout targets
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_td_window.h: TdwList and kTdwWaves are there); not a
// standalone header.
#pragma once

namespace {

// narde_value_fit: theta += alpha sum_i G_i grad v(s_i) over given records
// and given float targets, G_i = w_i (target_i - v_i).  A regression's error
// is local to its sample, so the windowed update's values pass, returns pass
// and second forward are one forward here:
//   k_fit_grad   k_tdw_grad's slab, accumulator and two stage sets; the
//                forwarding wave forms G_i from td_forward<true>'s own return
//                value, stores v[i], and hands w_i and e_i to the thread that
//                owns b2's element, which keeps the slab's loss in double;
//   k_td_update  (kernels_td.h) the partial rows in slab order;
//   k_fit_loss   the slabs' losses in slab order (only where the caller asks).
// No float atomics, and the windowed update's summation order.  k_fit_grad
// restates k_tdw_grad's loop instead of sharing it: with the list fill and the
// adds as shared inline functions the compiler schedules k_tdw_grad differently
// (DESIGN.md 24.2), and that kernel's code is to stay as it is.
static_assert(kFitSlab == NARDE_VALUE_FIT_SLAB, "narde.h and narde_rules.h state the same slab");
static_assert(kFitSlab == kTdwSlab, "the windowed update's slabs: the same sums, the same bits");

__global__ void __launch_bounds__(2 * kTdBlock) k_fit_grad(const uint4* __restrict__ records, int64_t samples,
                                                           TdNet net, const float* __restrict__ target,
                                                           const float* __restrict__ weight, float* __restrict__ part,
                                                           int64_t ld_part, double* __restrict__ slab_loss,
                                                           float* __restrict__ v) {
  extern __shared__ float4 fit_lds[];
  float* const acc = reinterpret_cast<float*>(fit_lds);
  __shared__ TdStage S[2][kTdwWaves];
  __shared__ TdwList W[2][kTdwWaves];
  __shared__ float2 WE[2][kTdwWaves];  // a staged sample's loss weight and error, for b2's owner
  const int H = net.hidden;
  const int P = kTdCols * H + 1;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool forwards = wave < kTdwWaves;  // wave-uniform
  const int classes = kTdBlock / H;        // 2 at least
  const int t = tid - kTdBlock, g = t / H, h = t - g * H;  // (the accumulating threads')
  const int64_t i0 = (int64_t)blockIdx.x * kFitSlab;
  const int ns = (int)min((int64_t)kFitSlab, samples - i0);
  const int nbatch = (ns + kTdwWaves - 1) / kTdwWaves;
  double se = 0.0, sw = 0.0;  // (thread t == 0's: the slab's loss)
  for (int p = tid; p < P; p += 2 * kTdBlock) acc[p] = 0.0f;
  for (int b = 0; b <= nbatch; ++b) {
    __syncthreads();  // the zeroes; batch b - 1 is staged, batch b - 2 is added
    if (forwards) {
      const int j = b * kTdwWaves + wave;
      if (j < ns) {  // wave-uniform
        const int64_t i = i0 + j;
        const uint4 ra = records[2 * i], rb = records[2 * i + 1];
        TdwList& L = W[b & 1][wave];
        const float val = td_forward<true>(net, S[b & 1][wave], ra, rb, lane);
        // the columns by slot, as td_forward placed their values in S.cols.xv
        int col[4];
        float xval[4];
        const int c = tes_item_nonzero(ra, rb, lane, col, xval);
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
          float w, e;
          L.G = fit_gain(target, weight, i, val, w, e);
          WE[b & 1][wave] = make_float2(w, e);
          if (v) v[i] = val;
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
        if (t == 0) {
          acc[P - 1] = tdw_acc_b2(acc[P - 1], Gs, T.go);
          const float2 we = WE[(b - 1) & 1][w];
          fit_loss_add(se, sw, we.x, we.y);
        }
      }
    }
  }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * ld_part;
  for (int p = tid; p < P; p += 2 * kTdBlock) out[p] = acc[p];
  if (t == 0) {
    slab_loss[2 * (int64_t)blockIdx.x] = se;
    slab_loss[2 * (int64_t)blockIdx.x + 1] = sw;
  }
}

// loss = the slabs' {sum w e^2, sum w} added in slab order (one thread: one order)
__global__ void __launch_bounds__(64) k_fit_loss(const double* __restrict__ slab_loss, int slabs,
                                                 double* __restrict__ loss) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double se = 0.0, sw = 0.0;
  for (int s = 0; s < slabs; ++s) {
    se += slab_loss[2 * (int64_t)s];
    sw += slab_loss[2 * (int64_t)s + 1];
  }
  loss[0] = se;
  loss[1] = sw;
}

// narde_playout_targets: a thread a root
__global__ void __launch_bounds__(kBlock) k_playout_targets(int64_t n, int trials, const int32_t* __restrict__ sums,
                                                            const float* __restrict__ leaf,
                                                            const uint32_t* __restrict__ roots,
                                                            float* __restrict__ target, float* __restrict__ weight) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float tg, wt;
  playout_target(sums + 4 * i, leaf ? leaf + i * trials : nullptr, trials, roots ? roots + 8 * i : nullptr, tg, wt);
  target[i] = tg;
  weight[i] = wt;
}

}  // namespace
