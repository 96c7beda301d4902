// kernels_td.h -- TD(lambda) on the value MLP
// Part of the one translation unit narde.hip (included there, in order);
// not a standalone header.
#pragma once

namespace {

// narde_value_td_trace: k_td_trace, one env a workgroup -- wave 0 evaluates
// the net on the env's record (the scored fills' forward: narde_rules.h
// "value MLP", the same lane and unit split) and leaves the units' gradient
// pieces in LDS, then the workgroup streams the env's trace row through once,
// float4 a lane: decay everywhere, the W1 bump on the record's own columns.
// narde_value_td_apply: k_td_delta (a wave an env: the successor's value
// under the weights as they are, the TD error), k_td_partial (kTdSlab envs a
// partial row: sum of delta x trace in env order; done envs' rows zeroed
// behind the read), k_td_update (the partial rows in slab order, into the
// weights and the mirror).  No float atomics: the sums have one order.
// The row streams are plain float4 loads and stores: non-temporal loads and
// stores cost 30 % at B = 4,096 (the apply pass then misses the rows the
// trace pass has just written), non-temporal loads alone 6 % there and gain
// 1-2 % at 16,384.
constexpr int kTdBlock = 256;

struct TdNet {
  float* w1t;  // [198][ld]
  int64_t ld;
  float* b1;
  float* w2;
  float* b2;
  float* w1;  // [hidden][ld_w1] mirror, or NULL
  int64_t ld_w1;
  int hidden, hidden_act, out_act;
};

struct alignas(16) TdStage {  // per forward wave
  uint2 root[kValRootSlots];  // the env's own columns
  TdCols cols;
  float d[kValHiddenMax], ga[kValHiddenMax];  // td_unit_grad's pieces, by unit
  float go;
};

// p / hidden for p < 2^15 by one multiply: m = ceil(2^32 / hidden)
__device__ __forceinline__ uint64_t td_div_magic(int hidden) {
  return ((uint64_t(1) << 32) + (uint64_t)hidden - 1u) / (uint64_t)hidden;
}
__device__ __forceinline__ int td_div(int p, uint64_t m) { return (int)(((uint64_t)(uint32_t)p * m) >> 32); }

// v(record) by one wave (all lanes, the same record); kGrad: the column mask
// and the units' gradient pieces are left in S for the lanes that follow a
// barrier
template <bool kGrad>
__device__ __forceinline__ float td_forward(const TdNet& n, TdStage& S, const uint4& ra, const uint4& rb, int lane) {
  const int t = lane & (kValLanes - 1), g = lane / kValLanes;
  const int nu = (n.hidden + kValLanes - 1) / kValLanes;
  int col[4];
  float val[4];
  const int c = tes_item_nonzero(ra, rb, lane, col, val);
  const int incl = wave_scan_incl(c, lane);
  const int total = min(__builtin_amdgcn_readlane(incl, 63), kValRootSlots);  // 33 at most; the bounds guard
  const int npad = (total + kValRootBatch - 1) / kValRootBatch * kValRootBatch;
  if (kGrad && lane < kTdMaskWords) S.cols.mask[lane] = 0u;
  wave_lds_handoff();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = incl - c + j;
    if (j < c && k < kValRootSlots) {
      S.root[k] = val_entry(col[j], val[j], n.ld);
      if (kGrad) {
        S.cols.xv[k] = val[j];
        atomicOr(&S.cols.mask[col[j] >> 5], 1u << (col[j] & 31));  // (LDS; an OR has no order)
      }
    }
  }
  if (total + lane < npad) S.root[total + lane] = make_uint2(0u, 0u);
  wave_lds_handoff();
  if (kGrad && lane == 0) td_cols_prefix(S.cols);
  float v = 0.0f;
  val_units(nu, [&](auto NU) {
    float z[kValUnits], w2t[kValUnits], a[kValUnits];
    val_root_part<NU.value>(S.root, npad, g, n.w1t, t, n.hidden, z);
#pragma unroll
    for (int i = 0; i < NU.value; ++i) {
      const bool on = t + kValLanes * i < n.hidden;
      const float pair = z[i] + __shfl_xor(z[i], kValLanes, 64);
      z[i] = (pair + __shfl_xor(pair, 2 * kValLanes, 64)) + (on ? n.b1[t + kValLanes * i] : 0.0f);
      w2t[i] = on ? n.w2[t + kValLanes * i] : 0.0f;
    }
    float part = val_lane_acts<NU.value>(z, w2t, n.hidden_act, a);
#pragma unroll
    for (int o = kValLanes / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    v = val_out_act(n.b2[0] + part, n.out_act);
    if (kGrad) {
      const float go = val_out_slope(v, n.out_act);
      if (lane == 0) S.go = go;
#pragma unroll
      for (int i = 0; i < NU.value; ++i) {
        const int h = t + kValLanes * i;
        if (g == 0 && h < n.hidden) td_unit_grad(go, w2t[i], z[i], a[i], n.hidden_act, S.ga[h], S.d[h]);
      }
    }
  });
  return v;
}

__global__ void __launch_bounds__(kTdBlock) k_td_trace(Planes pl, int n, TdNet net, float decay,
                                                       float* __restrict__ trace, int64_t ld_trace,
                                                       float* __restrict__ v, uint8_t* __restrict__ black) {
  __shared__ TdStage S;
  const int e = blockIdx.x;
  if (e >= n) return;  // (workgroup-uniform; the grid is n workgroups)
  if (threadIdx.x < 64) {
    const uint4 ra = pl.p0[e], rb = pl.p1[e];
    const float val = td_forward<true>(net, S, ra, rb, (int)threadIdx.x);
    if (threadIdx.x == 0) {
      v[e] = val;
      black[e] = (uint8_t)((rb.z >> 10) & 1u);
    }
  }
  __syncthreads();
  const int H = net.hidden;
  const int nq = (kTdCols / 4) * H;  // the row's float4 pieces; one float follows them
  const uint64_t m = td_div_magic(H);
  float* row = trace + (int64_t)e * ld_trace;
  float4* row4 = reinterpret_cast<float4*>(row);
  const bool keep = decay != 0.0f;  // kernel-uniform
#pragma unroll 4
  for (int q = (int)threadIdx.x; q < nq; q += kTdBlock) {
    int c = td_div(4 * q, m), h = 4 * q - c * H;
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (keep) o = row4[q];
    float r[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gr = 0.0f;
      const bool hit = td_grad_at(c, h, S.cols, S.d, S.ga, S.go, gr);
      r[j] = td_trace_at(decay, r[j], hit, gr);
      if (++h == H) h = 0, ++c;
    }
    row4[q] = make_float4(r[0], r[1], r[2], r[3]);
  }
  if (threadIdx.x == 0) {  // b2's
    const int p = kTdCols * H;
    row[p] = td_trace_at(decay, keep ? row[p] : 0.0f, true, S.go);
  }
}

__global__ void __launch_bounds__(kTdBlock) k_td_delta(Planes pl, int n, TdNet net, const float* __restrict__ v,
                                                       const uint8_t* __restrict__ black,
                                                       const int32_t* __restrict__ reward,
                                                       const uint8_t* __restrict__ terminated,
                                                       const uint8_t* __restrict__ truncated, float gamma,
                                                       float* __restrict__ dl, float* __restrict__ delta) {
  __shared__ TdStage S[kTdBlock / 64];
  const int e = aft_wave_env(kTdBlock / 64);
  if (e >= n) return;
  const bool tm = terminated[e] != 0, tr = truncated[e] != 0;  // wave-uniform
  float vn = 0.0f;
  if (!tm && !tr) vn = td_forward<false>(net, S[threadIdx.x >> 6], pl.p0[e], pl.p1[e], (int)(threadIdx.x & 63));
  if ((threadIdx.x & 63) == 0) {
    const float d = td_delta(tm, tr, reward[e], black[e], gamma, vn, v[e]);
    dl[e] = d;
    if (delta) delta[e] = d;
  }
}

__device__ __forceinline__ void td_fma4(float s, const float4& t, float4& acc) {
  acc.x = fmaf(s, t.x, acc.x);
  acc.y = fmaf(s, t.y, acc.y);
  acc.z = fmaf(s, t.z, acc.z);
  acc.w = fmaf(s, t.w, acc.w);
}

// grid (the row's pieces / kTdBlock, slabs): part[slab][p] = sum over the
// slab's envs, in env order, of dl[e] trace[e][p]
__global__ void __launch_bounds__(kTdBlock) k_td_partial(int n, int hidden, float* __restrict__ trace,
                                                         int64_t ld_trace, const float* __restrict__ dl,
                                                         const uint8_t* __restrict__ terminated,
                                                         const uint8_t* __restrict__ truncated,
                                                         float* __restrict__ part, int64_t ld_part) {
  __shared__ float sd[kTdSlab];
  __shared__ uint8_t sz[kTdSlab];
  const int e0 = (int)blockIdx.y * kTdSlab;
  const int ne = min(kTdSlab, n - e0);
  if (threadIdx.x < kTdSlab) {
    const int k = (int)threadIdx.x;
    const bool in = k < ne;
    sd[k] = in ? dl[e0 + k] : 0.0f;  // (0 past the last env: such a term adds nothing)
    sz[k] = in && (terminated[e0 + k] != 0 || truncated[e0 + k] != 0);
  }
  __syncthreads();
  const int nq = (kTdCols / 4) * hidden;
  const int q = (int)(blockIdx.x * kTdBlock + threadIdx.x);
  float* rows = trace + (int64_t)e0 * ld_trace;
  float* out = part + (int64_t)blockIdx.y * ld_part;
  constexpr int kB = 8;  // loads in flight a lane
  static_assert(kTdSlab % kB == 0, "whole batches");
  if (q < nq) {
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k0 = 0; k0 < ne; k0 += kB) {
      float4 t[kB];
#pragma unroll
      for (int j = 0; j < kB; ++j)
        t[j] = k0 + j < ne ? reinterpret_cast<const float4*>(rows + (int64_t)(k0 + j) * ld_trace)[q]
                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int j = 0; j < kB; ++j) td_fma4(sd[k0 + j], t[j], acc);
#pragma unroll
      for (int j = 0; j < kB; ++j)
        if (sz[k0 + j]) reinterpret_cast<float4*>(rows + (int64_t)(k0 + j) * ld_trace)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    reinterpret_cast<float4*>(out)[q] = acc;
  } else if (q == nq) {  // b2's
    const int p = kTdCols * hidden;
    float acc = 0.0f;
    for (int k = 0; k < ne; ++k) {
      float* x = rows + (int64_t)k * ld_trace + p;
      acc = fmaf(sd[k], *x, acc);
      if (sz[k]) *x = 0.0f;
    }
    out[p] = acc;
  }
}

// theta[p] += alpha x (the partial rows' sum, in slab order)
__global__ void __launch_bounds__(kTdBlock) k_td_update(TdNet net, float alpha, const float* __restrict__ part,
                                                        int64_t ld_part, int slabs) {
  const int H = net.hidden;
  const int p = (int)(blockIdx.x * kTdBlock + threadIdx.x);
  if (p > kTdCols * H) return;
  constexpr int kB = 8;
  float sum = 0.0f;
  for (int s0 = 0; s0 < slabs; s0 += kB) {
    float t[kB];
#pragma unroll
    for (int j = 0; j < kB; ++j) t[j] = s0 + j < slabs ? part[(int64_t)(s0 + j) * ld_part + p] : 0.0f;
#pragma unroll
    for (int j = 0; j < kB; ++j) sum += t[j];
  }
  const int c = td_div(p, td_div_magic(H)), h = p - c * H;
  if (c < kTdColB1) {
    float* w = net.w1t + (int64_t)c * net.ld + h;
    const float x = fmaf(alpha, sum, *w);
    *w = x;
    if (net.w1) net.w1[(int64_t)h * net.ld_w1 + c] = x;
  } else {
    float* w = c == kTdColB1 ? net.b1 + h : (c == kTdColW2 ? net.w2 + h : net.b2);
    *w = fmaf(alpha, sum, *w);
  }
}

}  // namespace
