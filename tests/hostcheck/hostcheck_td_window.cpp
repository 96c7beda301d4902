// hostcheck_td_window.cpp -- TEST-ONLY host build of the windowed TD(lambda)
// arithmetic (gym-narde_amd/csrc/narde_rules.h "windowed TD(lambda)" on top
// of "TD(lambda)" and "value MLP").
//
// Runs the functions narde_value_td_window's kernels (kernels_td_window.h)
// run, serially and in their summation order: the values pass a sample at a
// time (the forward 16 lanes a lane group in the wave's order), the returns
// pass backward over k per env, the gradient pass a slab of kTdwSlab samples
// at a time into one dense accumulator -- an element takes one addend a
// sample, in sample order --, and k_td_update's fold of the partial rows in
// slab order.  tests/test_td_window_cpu.py compares v, delta, G and the
// updated weights with torch in float64.  Never loaded by the product.
#include <cstring>
#include <vector>

#include "../../gym-narde_amd/csrc/narde_rules.h"
#include "../../include/narde.h"

using namespace narde;

namespace {

struct Forward {
  float v, go;
  float d[kValHiddenMax], ga[kValHiddenMax];
};

// hostcheck_td.cpp's forward: v and the units' gradient pieces of one record
void forward(const uint4& ra, const uint4& rb, const float* w1t, int64_t ld, const float* b1, const float* w2,
             const float* b2, int hidden, int hidden_act, int out_act, Forward& F) {
  const int nu = (hidden + kValLanes - 1) / kValLanes;
  uint2 root[kValRootSlots];
  const int nroot = val_root_list(ra, rb, ld, root);
  float z[kValLanes][kValUnits], a[kValLanes][kValUnits], w2t[kValLanes][kValUnits], part[kValLanes], next[kValLanes];
  for (int t = 0; t < kValLanes; ++t) {
    float p[kValRows][kValUnits];
    val_units(nu, [&](auto NU) {
      for (int g = 0; g < kValRows; ++g) val_root_part<NU.value>(root, nroot, g, w1t, t, hidden, p[g]);
      for (int i = 0; i < kValUnits; ++i) {
        const bool on = i < nu && t + kValLanes * i < hidden;
        z[t][i] = i < nu ? ((p[0][i] + p[1][i]) + (p[2][i] + p[3][i])) + (on ? b1[t + kValLanes * i] : 0.0f) : 0.0f;
        w2t[t][i] = on ? w2[t + kValLanes * i] : 0.0f;
      }
      part[t] = val_lane_acts<NU.value>(z[t], w2t[t], hidden_act, a[t]);
    });
  }
  for (int o = kValLanes / 2; o > 0; o >>= 1) {
    for (int t = 0; t < kValLanes; ++t) next[t] = part[t] + part[t ^ o];
    memcpy(part, next, sizeof part);
  }
  F.v = val_out_act(b2[0] + part[0], out_act);
  F.go = val_out_slope(F.v, out_act);
  for (int h = 0; h < hidden; ++h) {
    const int t = h % kValLanes, i = h / kValLanes;
    td_unit_grad(F.go, w2t[t][i], z[t][i], a[t][i], hidden_act, F.ga[h], F.d[h]);
  }
}

}  // namespace

extern "C" {

int hc_tdw_slab(void) { return kTdwSlab; }
int hc_tdw_slab_macro(void) { return NARDE_TD_WINDOW_SLAB; }
int64_t hc_tdw_scratch_floats(int64_t n, int plies, int hidden) { return tdw_scratch_floats(n, plies, hidden); }
int64_t hc_tdw_scratch_macro(int64_t n, int plies, int hidden) { return NARDE_TD_WINDOW_SCRATCH_FLOATS(n, plies, hidden); }

// A window of K plies of B envs: states (board i8[24] absolute, off u8[2],
// player i8) for the (K + 1) B samples k B + e, the last B the envs' records
// as they stand; reward i32, terminated, truncated u8 [K][B]; the net (w1t
// f32[198][ld], b1, w2 f32[hidden], b2 f32[1]), updated in place.  Out:
// v f32[(K + 1) B], delta and G f32[K B].
void hc_td_window(int K, int64_t B, const int8_t* board, const uint8_t* off, const int8_t* player,
                  const int32_t* reward, const uint8_t* terminated, const uint8_t* truncated, float* w1t, int64_t ld,
                  float* b1, float* w2, float* b2, int hidden, int hidden_act, int out_act, float alpha, float lam,
                  float gamma, float* v, float* delta, float* G) {
  const int64_t stored = (int64_t)K * B, all = stored + B;
  std::vector<uint4> ra(all), rb(all);
  Forward F;
  // k_tdw_values
  for (int64_t i = 0; i < all; ++i) {
    record_from_board(board + 24 * i, off[2 * i], off[2 * i + 1], 0u, 0u, player[i], 0u, 0u, ra[i], rb[i]);
    forward(ra[i], rb[i], w1t, ld, b1, w2, b2, hidden, hidden_act, out_act, F);
    v[i] = F.v;
  }
  // k_tdw_returns
  const float gl = gamma * lam;
  for (int64_t e = 0; e < B; ++e) {
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
  // k_tdw_grad: a partial row a slab
  const int64_t P = td_row_floats(hidden), slabs = tdw_slabs(stored);
  std::vector<float> part((size_t)(slabs * P), 0.0f);
  for (int64_t s = 0; s < slabs; ++s) {
    float* acc = part.data() + s * P;
    const int64_t i1 = (s + 1) * kTdwSlab < stored ? (s + 1) * kTdwSlab : stored;
    for (int64_t i = s * kTdwSlab; i < i1; ++i) {
      forward(ra[i], rb[i], w1t, ld, b1, w2, b2, hidden, hidden_act, out_act, F);
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
  // k_td_update: the partial rows in slab order
  for (int64_t p = 0; p < P; ++p) {
    float sum = 0.0f;
    for (int64_t s = 0; s < slabs; ++s) sum += part[(size_t)(s * P + p)];
    const int c = (int)(p / hidden), h = (int)(p - (int64_t)c * hidden);
    float* w = c < kTdColB1 ? w1t + (int64_t)c * ld + h : (c == kTdColB1 ? b1 + h : (c == kTdColW2 ? w2 + h : b2));
    *w = fmaf(alpha, sum, *w);
  }
}

}  // extern "C"
