// kernels_value_optim.h -- the value updates' gradient and optimiser steps on it
// Part of the one translation unit narde.hip (included there, in order, behind
// kernels_value_fit.h: TdNet, td_div and kTdBlock are kernels_td.h's); not a
// standalone header.
#pragma once

namespace {

// narde_value_td_window_grad / narde_value_fit_grad: the plain calls' kernels
// up to the partial rows, then
//   k_td_fold    k_td_update's summation loop -- the partial rows in slab
//                order, from 0.0f, in its batches -- with a store of the sum
//                in place of the apply: grad[p] is the `sum` that kernel forms.
// The steps on a given gradient, a thread an element of the row:
//   k_opt_norm   one workgroup: the squares in double, a lane's elements in
//                index order, the lanes by halving; the norm and the clip
//                coefficient;
//   k_sgd_step   theta = fmaf(alpha, g, theta) -- k_td_update's apply;
//   k_adam_tick  one thread: the step count and the running products;
//   k_adam_step  AdamW's element, every thread reading the state the tick
//                launch in front of it left.
// The steps write w1t and the mirror the same bits, as k_td_update does.  No
// float atomics anywhere: every element has one owner, every sum one order.
static_assert(sizeof(AdamState) == sizeof(narde_adam_state), "narde.h and narde_rules.h state the same struct");
static_assert(offsetof(AdamState, b1t) == offsetof(narde_adam_state, beta1_pow) &&
                  offsetof(AdamState, b2t) == offsetof(narde_adam_state, beta2_pow),
              "narde.h and narde_rules.h state the same struct");
static_assert(kTdCols * kValHiddenMax + 1 < (1 << 15), "td_div's range");

__global__ void __launch_bounds__(kTdBlock) k_td_fold(int P, const float* __restrict__ part, int64_t ld_part,
                                                      int slabs, float* __restrict__ grad) {
  const int p = (int)(blockIdx.x * kTdBlock + threadIdx.x);
  if (p >= P) return;
  constexpr int kB = 8;
  float sum = 0.0f;
  for (int s0 = 0; s0 < slabs; s0 += kB) {
    float t[kB];
#pragma unroll
    for (int j = 0; j < kB; ++j) t[j] = s0 + j < slabs ? part[(int64_t)(s0 + j) * ld_part + p] : 0.0f;
#pragma unroll
    for (int j = 0; j < kB; ++j) sum += t[j];
  }
  grad[p] = sum;
}

// element p's weight, and its place in the mirror (NULL: none)
__device__ __forceinline__ float* opt_slot(const TdNet& net, int p, float*& mirror) {
  const int H = net.hidden;
  const int c = td_div(p, td_div_magic(H)), h = p - c * H;
  mirror = nullptr;
  if (c < kTdColB1) {
    if (net.w1) mirror = net.w1 + (int64_t)h * net.ld_w1 + c;
    return net.w1t + (int64_t)c * net.ld + h;
  }
  return c == kTdColB1 ? net.b1 + h : (c == kTdColW2 ? net.w2 + h : net.b2);
}

__global__ void __launch_bounds__(kOptBlock) k_opt_norm(int P, const float* __restrict__ grad, float max_norm,
                                                        float* __restrict__ out) {
  __shared__ double lanes[kOptBlock];
  if (blockIdx.x != 0) return;  // (workgroup-uniform; the grid is one workgroup)
  const int l = (int)threadIdx.x;
  double acc = 0.0;
  for (int p = l; p < P; p += kOptBlock) acc = opt_sq_add(acc, grad[p]);
  lanes[l] = acc;
  __syncthreads();
  for (int o = kOptBlock / 2; o > 0; o >>= 1) {
    if (l < o) lanes[l] += lanes[l + o];
    __syncthreads();
  }
  if (l == 0) {
    float norm, scale;
    opt_norm_finish(lanes[0], max_norm, norm, scale);
    out[0] = norm;
    out[1] = scale;
  }
}

__global__ void __launch_bounds__(kTdBlock) k_sgd_step(TdNet net, const float* __restrict__ grad,
                                                       const float* __restrict__ scale, float alpha) {
  const int p = (int)(blockIdx.x * kTdBlock + threadIdx.x);
  if (p > kTdCols * net.hidden) return;
  float* mirror;
  float* w = opt_slot(net, p, mirror);
  const float x = sgd_element(*w, opt_grad(grad[p], scale), alpha);
  *w = x;
  if (mirror) *mirror = x;
}

__global__ void __launch_bounds__(64) k_adam_tick(AdamState* __restrict__ state, float beta1, float beta2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  AdamState S = *state;
  adam_tick(S, beta1, beta2);
  *state = S;
}

__global__ void __launch_bounds__(kTdBlock) k_adam_step(TdNet net, const float* __restrict__ grad,
                                                        const float* __restrict__ scale, float* __restrict__ m,
                                                        float* __restrict__ s, const AdamState* __restrict__ state,
                                                        float lr, float beta1, float beta2, float eps, float keep) {
  const int p = (int)(blockIdx.x * kTdBlock + threadIdx.x);
  if (p > kTdCols * net.hidden) return;
  float step_size, bc2_sqrt;
  adam_coeffs(*state, lr, step_size, bc2_sqrt);  // (kernel-uniform)
  float* mirror;
  float* w = opt_slot(net, p, mirror);
  float mp = m[p], sp = s[p];
  const float x = adam_element(*w, opt_grad(grad[p], scale), mp, sp, keep, beta1, beta2, step_size, bc2_sqrt, eps);
  m[p] = mp;
  s[p] = sp;
  *w = x;
  if (mirror) *mirror = x;
}

}  // namespace
