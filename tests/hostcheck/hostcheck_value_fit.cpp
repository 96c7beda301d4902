// hostcheck_value_fit.cpp -- TEST-ONLY host build of the supervised fit's and
// the playout targets' arithmetic (gym-narde_amd/csrc/narde_rules.h "the value
// MLP's supervised fit" on top of "windowed TD(lambda)", "TD(lambda)" and
// "value MLP").
//
// Runs the functions narde_value_fit's kernels (kernels_value_fit.h) run,
// serially and in their summation order: a slab of kFitSlab samples at a time
// -- one forward a sample (16 lanes a lane group in the wave's order), G from
// that forward's own value, the dense accumulator taking one addend an element
// a sample in sample order, the slab's loss in double beside it --, then
// k_td_update's fold of the partial rows in slab order into the weights and the
// mirror, and k_fit_loss's fold of the slabs' losses.  The scratch is laid out
// as the call lays it out.  tests/test_value_fit_cpu.py compares v and the
// updated weights with torch in float64.  Never loaded by the product.
#include <cstring>

#include "../../gym-narde_amd/csrc/narde_rules.h"
#include "../../include/narde.h"

using namespace narde;

namespace {

struct Forward {
  float v, go;
  float d[kValHiddenMax], ga[kValHiddenMax];
};

// hostcheck_td_window.cpp's forward: v and the units' gradient pieces of one record
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

int hc_fit_slab(void) { return kFitSlab; }
int hc_fit_slab_macro(void) { return NARDE_VALUE_FIT_SLAB; }
int64_t hc_fit_scratch_floats(int64_t n, int hidden) { return fit_scratch_floats(n, hidden); }
int64_t hc_fit_scratch_macro(int64_t n, int hidden) { return NARDE_VALUE_FIT_SCRATCH_FLOATS(n, hidden); }

// n samples: states (board i8[24] absolute, off u8[2], player i8), target f32[n],
// weight f32[n] or NULL; the net (w1t f32[198][ld], b1, w2 f32[hidden], b2
// f32[1]; w1 f32[hidden][ld_w1] the mirror, or NULL), updated in place;
// scratch f32[fit_scratch_floats(n, hidden)] at least, 8-B aligned.  Out (each
// optional): v f32[n], loss f64[2].
void hc_value_fit(int64_t n, const int8_t* board, const uint8_t* off, const int8_t* player, const float* target,
                  const float* weight, float* w1t, int64_t ld, float* b1, float* w2, float* b2, int hidden,
                  int hidden_act, int out_act, float* w1, int64_t ld_w1, float alpha, float* scratch, float* v,
                  double* loss) {
  const int64_t P = td_row_floats(hidden), ld_part = P + 3, slabs = tdw_slabs(n);
  float* part = scratch;
  double* slab_loss = reinterpret_cast<double*>(scratch + slabs * ld_part);
  Forward F;
  // k_fit_grad: a partial row and a loss a slab
  for (int64_t s = 0; s < slabs; ++s) {
    float* acc = part + s * ld_part;
    for (int64_t p = 0; p < P; ++p) acc[p] = 0.0f;
    double se = 0.0, sw = 0.0;
    const int64_t i1 = (s + 1) * kFitSlab < n ? (s + 1) * kFitSlab : n;
    for (int64_t i = s * kFitSlab; i < i1; ++i) {
      uint4 ra, rb;
      record_from_board(board + 24 * i, off[2 * i], off[2 * i + 1], 0u, 0u, player[i], 0u, 0u, ra, rb);
      forward(ra, rb, w1t, ld, b1, w2, b2, hidden, hidden_act, out_act, F);
      float w, e;
      const float G = fit_gain(target, weight, i, F.v, w, e);
      if (v) v[i] = F.v;
      TdCols C;
      td_cols_of(ra, rb, C);
      int q = 0;
      for (int c = 0; c < kTdColB1; ++c) {
        if (!((C.mask[c >> 5] >> (c & 31)) & 1u)) continue;
        for (int h = 0; h < hidden; ++h) acc[c * hidden + h] = tdw_acc(acc[c * hidden + h], G, c, C.xv[q], F.d[h], F.ga[h]);
        ++q;
      }
      for (int c = kTdColB1; c < kTdCols; ++c)
        for (int h = 0; h < hidden; ++h) acc[c * hidden + h] = tdw_acc(acc[c * hidden + h], G, c, 1.0f, F.d[h], F.ga[h]);
      acc[P - 1] = tdw_acc_b2(acc[P - 1], G, F.go);
      fit_loss_add(se, sw, w, e);
    }
    slab_loss[2 * s] = se;
    slab_loss[2 * s + 1] = sw;
  }
  // k_td_update: the partial rows in slab order, into the weights and the mirror
  for (int64_t p = 0; p < P; ++p) {
    float sum = 0.0f;
    for (int64_t s = 0; s < slabs; ++s) sum += part[s * ld_part + p];
    const int c = (int)(p / hidden), h = (int)(p - (int64_t)c * hidden);
    float* x = c < kTdColB1 ? w1t + (int64_t)c * ld + h : (c == kTdColB1 ? b1 + h : (c == kTdColW2 ? w2 + h : b2));
    *x = fmaf(alpha, sum, *x);
    if (c < kTdColB1 && w1) w1[(int64_t)h * ld_w1 + c] = *x;
  }
  // k_fit_loss: the slabs in slab order
  if (loss) {
    double se = 0.0, sw = 0.0;
    for (int64_t s = 0; s < slabs; ++s) {
      se += slab_loss[2 * s];
      sw += slab_loss[2 * s + 1];
    }
    loss[0] = se;
    loss[1] = sw;
  }
}

// k_playout_targets: a root at a time.  sums i32[n][4], leaf f32[n][trials] or
// NULL, roots u32[n][8] or NULL -> target, weight f32[n].
void hc_playout_targets(int64_t n, int trials, const int32_t* sums, const float* leaf, const uint32_t* roots,
                        float* target, float* weight) {
  for (int64_t i = 0; i < n; ++i)
    playout_target(sums + 4 * i, leaf ? leaf + i * trials : nullptr, trials, roots ? roots + 8 * i : nullptr, target[i],
                   weight[i]);
}

}  // extern "C"
