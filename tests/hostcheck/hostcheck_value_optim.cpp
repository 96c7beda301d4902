// hostcheck_value_optim.cpp -- TEST-ONLY host build of the gradient forms of
// the two batch updates and of the optimiser steps on a given gradient
// (gym-narde_amd/csrc/narde_rules.h "optimiser steps on a given gradient" on
// top of "the value MLP's supervised fit", "windowed TD(lambda)", "TD(lambda)"
// and "value MLP").
//
// Runs the functions the kernels of kernels_value_optim.h run, serially and in
// their order: k_td_fold's sum of the partial rows in slab order behind the
// windowed update's and the fit's own passes (hostcheck_td_window.cpp's and
// hostcheck_value_fit.cpp's, restated: a values pass, the gains, one
// accumulator a slab), k_opt_norm's lanes and halving, k_sgd_step's and
// k_adam_step's element behind k_adam_tick.  tests/test_value_optim_cpu.py
// compares them with tests/optim_ref.py in float64 and, through the SGD
// element, with the plain updates' host checks bit for bit.  Never loaded by
// the product.
#include <cstring>
#include <vector>

#include "../../include/narde.h"
#include "../../gym-narde_amd/csrc/narde_rules.h"

using namespace narde;

static_assert(sizeof(AdamState) == sizeof(narde_adam_state), "narde.h and narde_rules.h state the same struct");

namespace {

struct Forward {
  float v, go;
  float d[kValHiddenMax], ga[kValHiddenMax];
};

struct Net {
  float* w1t;
  int64_t ld;
  float *b1, *w2, *b2;
  int hidden, hidden_act, out_act;
  float* w1;
  int64_t ld_w1;
};

// hostcheck_td_window.cpp's forward: v and the units' gradient pieces of one record
void forward(const uint4& ra, const uint4& rb, const Net& n, Forward& F) {
  const int hidden = n.hidden, nu = (hidden + kValLanes - 1) / kValLanes;
  uint2 root[kValRootSlots];
  const int nroot = val_root_list(ra, rb, n.ld, root);
  float z[kValLanes][kValUnits], a[kValLanes][kValUnits], w2t[kValLanes][kValUnits], part[kValLanes], next[kValLanes];
  for (int t = 0; t < kValLanes; ++t) {
    float p[kValRows][kValUnits];
    val_units(nu, [&](auto NU) {
      for (int g = 0; g < kValRows; ++g) val_root_part<NU.value>(root, nroot, g, n.w1t, t, hidden, p[g]);
      for (int i = 0; i < kValUnits; ++i) {
        const bool on = i < nu && t + kValLanes * i < hidden;
        z[t][i] = i < nu ? ((p[0][i] + p[1][i]) + (p[2][i] + p[3][i])) + (on ? n.b1[t + kValLanes * i] : 0.0f) : 0.0f;
        w2t[t][i] = on ? n.w2[t + kValLanes * i] : 0.0f;
      }
      part[t] = val_lane_acts<NU.value>(z[t], w2t[t], n.hidden_act, a[t]);
    });
  }
  for (int o = kValLanes / 2; o > 0; o >>= 1) {
    for (int t = 0; t < kValLanes; ++t) next[t] = part[t] + part[t ^ o];
    memcpy(part, next, sizeof part);
  }
  F.v = val_out_act(n.b2[0] + part[0], n.out_act);
  F.go = val_out_slope(F.v, n.out_act);
  for (int h = 0; h < hidden; ++h) {
    const int t = h % kValLanes, i = h / kValLanes;
    td_unit_grad(F.go, w2t[t][i], z[t][i], a[t][i], n.hidden_act, F.ga[h], F.d[h]);
  }
}

// k_tdw_grad / k_fit_grad (a partial row a slab of kTdwSlab samples, an element
// taking one addend a sample in sample order), then k_td_fold: the rows in slab
// order, from 0.0f
void slabs_and_fold(int64_t samples, const std::vector<uint4>& ra, const std::vector<uint4>& rb, const Net& n,
                    const float* G, float* grad) {
  const int hidden = n.hidden;
  const int64_t P = td_row_floats(hidden), slabs = tdw_slabs(samples);
  std::vector<float> part((size_t)(slabs * P), 0.0f);
  Forward F;
  for (int64_t s = 0; s < slabs; ++s) {
    float* acc = part.data() + s * P;
    const int64_t i1 = (s + 1) * kTdwSlab < samples ? (s + 1) * kTdwSlab : samples;
    for (int64_t i = s * kTdwSlab; i < i1; ++i) {
      forward(ra[i], rb[i], n, F);
      TdCols C;
      td_cols_of(ra[i], rb[i], C);
      int q = 0;
      for (int c = 0; c < kTdColB1; ++c) {
        if (!((C.mask[c >> 5] >> (c & 31)) & 1u)) continue;
        for (int h = 0; h < hidden; ++h) acc[c * hidden + h] = tdw_acc(acc[c * hidden + h], G[i], c, C.xv[q], F.d[h], F.ga[h]);
        ++q;
      }
      for (int c = kTdColB1; c < kTdCols; ++c)
        for (int h = 0; h < hidden; ++h) acc[c * hidden + h] = tdw_acc(acc[c * hidden + h], G[i], c, 1.0f, F.d[h], F.ga[h]);
      acc[P - 1] = tdw_acc_b2(acc[P - 1], G[i], F.go);
    }
  }
  for (int64_t p = 0; p < P; ++p) {
    float sum = 0.0f;
    for (int64_t s = 0; s < slabs; ++s) sum += part[(size_t)(s * P + p)];
    grad[p] = sum;
  }
}

// element p's weight, and its place in the mirror (NULL: none)
float* slot(const Net& n, int64_t p, float*& mirror) {
  const int c = (int)(p / n.hidden), h = (int)(p - (int64_t)c * n.hidden);
  mirror = nullptr;
  if (c < kTdColB1) {
    if (n.w1) mirror = n.w1 + (int64_t)h * n.ld_w1 + c;
    return n.w1t + (int64_t)c * n.ld + h;
  }
  return c == kTdColB1 ? n.b1 + h : (c == kTdColW2 ? n.w2 + h : n.b2);
}

}  // namespace

extern "C" {

int hc_opt_block(void) { return kOptBlock; }
int hc_opt_state_bytes(void) { return (int)sizeof(AdamState); }

// narde_value_td_window_grad: hc_td_window's arguments without alpha, the net
// read only.  Out: v f32[(K + 1) B], delta and G f32[K B], grad f32[200 hidden + 1].
void hc_td_window_grad(int K, int64_t B, const int8_t* board, const uint8_t* off, const int8_t* player,
                       const int32_t* reward, const uint8_t* terminated, const uint8_t* truncated, float* w1t,
                       int64_t ld, float* b1, float* w2, float* b2, int hidden, int hidden_act, int out_act, float lam,
                       float gamma, float* v, float* delta, float* G, float* grad) {
  const Net n{w1t, ld, b1, w2, b2, hidden, hidden_act, out_act, nullptr, 0};
  const int64_t stored = (int64_t)K * B, all = stored + B;
  std::vector<uint4> ra(all), rb(all);
  Forward F;
  for (int64_t i = 0; i < all; ++i) {  // k_tdw_values
    record_from_board(board + 24 * i, off[2 * i], off[2 * i + 1], 0u, 0u, player[i], 0u, 0u, ra[i], rb[i]);
    forward(ra[i], rb[i], n, F);
    v[i] = F.v;
  }
  const float gl = gamma * lam;
  for (int64_t e = 0; e < B; ++e) {  // k_tdw_returns
    float vn = v[stored + e], gn = 0.0f;
    for (int k = K - 1; k >= 0; --k) {
      const int64_t i = (int64_t)k * B + e;
      const bool tm = terminated[i] != 0, tr = truncated[i] != 0;
      const float d = td_delta(tm, tr, reward[i], (rb[i].z >> 10) & 1u, gamma, vn, v[i]);
      gn = td_return(d, tm || tr, gl, gn);
      delta[i] = d;
      G[i] = gn;
      vn = v[i];
    }
  }
  slabs_and_fold(stored, ra, rb, n, G, grad);
}

// narde_value_fit_grad: hc_value_fit's arguments without alpha and the scratch,
// the net read only.  Out: v f32[n], loss f64[2] (the slabs' losses in slab
// order), grad f32[200 hidden + 1].
void hc_value_fit_grad(int64_t n_samples, const int8_t* board, const uint8_t* off, const int8_t* player,
                       const float* target, const float* weight, float* w1t, int64_t ld, float* b1, float* w2,
                       float* b2, int hidden, int hidden_act, int out_act, float* v, double* loss, float* grad) {
  const Net n{w1t, ld, b1, w2, b2, hidden, hidden_act, out_act, nullptr, 0};
  std::vector<uint4> ra(n_samples), rb(n_samples);
  std::vector<float> G(n_samples);
  Forward F;
  double total_e = 0.0, total_w = 0.0, se = 0.0, sw = 0.0;
  for (int64_t i = 0; i < n_samples; ++i) {  // k_fit_grad's forward, gain and loss of a sample
    record_from_board(board + 24 * i, off[2 * i], off[2 * i + 1], 0u, 0u, player[i], 0u, 0u, ra[i], rb[i]);
    forward(ra[i], rb[i], n, F);
    float w, e;
    G[i] = fit_gain(target, weight, i, F.v, w, e);
    v[i] = F.v;
    fit_loss_add(se, sw, w, e);
    if ((i + 1) % kFitSlab == 0 || i + 1 == n_samples) {  // k_fit_loss: the slabs in slab order
      total_e += se;
      total_w += sw;
      se = sw = 0.0;
    }
  }
  loss[0] = total_e;
  loss[1] = total_w;
  slabs_and_fold(n_samples, ra, rb, n, G.data(), grad);
}

// k_opt_norm: lane l's elements in index order, then the lanes by halving
void hc_grad_norm(int hidden, const float* grad, float max_norm, float* out) {
  const int64_t P = td_row_floats(hidden);
  double lanes[kOptBlock];
  for (int l = 0; l < kOptBlock; ++l) {
    double acc = 0.0;
    for (int64_t p = l; p < P; p += kOptBlock) acc = opt_sq_add(acc, grad[p]);
    lanes[l] = acc;
  }
  for (int o = kOptBlock / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) lanes[l] += lanes[l + o];
  opt_norm_finish(lanes[0], max_norm, out[0], out[1]);
}

// k_sgd_step, an element at a time; scale f32[1] or NULL; w1 the mirror or NULL
void hc_sgd_step(float* w1t, int64_t ld, float* b1, float* w2, float* b2, int hidden, float* w1, int64_t ld_w1,
                 const float* grad, const float* scale, float alpha) {
  const Net n{w1t, ld, b1, w2, b2, hidden, 0, 0, w1, ld_w1};
  for (int64_t p = 0; p < td_row_floats(hidden); ++p) {
    float* mirror;
    float* w = slot(n, p, mirror);
    *w = sgd_element(*w, opt_grad(grad[p], scale), alpha);
    if (mirror) *mirror = *w;
  }
}

// k_adam_tick, then k_adam_step an element at a time; state: sizeof(AdamState)
// bytes, zero before the first step
void hc_adam_step(float* w1t, int64_t ld, float* b1, float* w2, float* b2, int hidden, float* w1, int64_t ld_w1,
                  const float* grad, const float* scale, float* m, float* s, void* state, float lr, float beta1,
                  float beta2, float eps, float weight_decay) {
  const Net n{w1t, ld, b1, w2, b2, hidden, 0, 0, w1, ld_w1};
  AdamState S;
  memcpy(&S, state, sizeof S);
  adam_tick(S, beta1, beta2);
  memcpy(state, &S, sizeof S);
  const float keep = 1.0f - lr * weight_decay;
  float step_size, bc2_sqrt;
  adam_coeffs(S, lr, step_size, bc2_sqrt);
  for (int64_t p = 0; p < td_row_floats(hidden); ++p) {
    float* mirror;
    float* w = slot(n, p, mirror);
    *w = adam_element(*w, opt_grad(grad[p], scale), m[p], s[p], keep, beta1, beta2, step_size, bc2_sqrt, eps);
    if (mirror) *mirror = *w;
  }
}

}  // extern "C"
