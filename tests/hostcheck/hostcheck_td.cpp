// hostcheck_td.cpp -- TEST-ONLY host build of the TD(lambda) arithmetic
// (gym-narde_amd/csrc/narde_rules.h "TD(lambda)" on top of "value MLP").
//
// Runs the functions k_td_trace (kernels_td.h) runs: the record's column
// list, the forward 16 lanes a lane group in the wave's order, the units'
// gradient pieces and the walk over a trace row, element by element.
// tests/test_td_cpu.py compares the values, the gradient rows and the trace
// updates with torch in float64.  Never loaded by the product.
#include <cstring>

#include "../../gym-narde_amd/csrc/narde_rules.h"

using namespace narde;

extern "C" {

int hc_td_slab(void) { return kTdSlab; }
int64_t hc_td_row_floats(int hidden) { return td_row_floats(hidden); }

// Per state r (board i8[24] absolute, off u8[2], player i8) and the net (w1t
// f32[198][ld], b1, w2 f32[hidden], b2 f32[1]): v[r], black[r] u8,
// trace[r] = decay trace[r] + grad v (f32[ld_trace] a row, floats past 200
// hidden + 1 untouched), cols u8[198] = 1 on the record's listed columns.
void hc_td_trace(int64_t n, const int8_t* board, const uint8_t* off, const int8_t* player, const float* w1t, int64_t ld,
                 const float* b1, const float* w2, const float* b2, int hidden, int hidden_act, int out_act,
                 float decay, float* trace, int64_t ld_trace, float* v, uint8_t* black, uint8_t* cols) {
  const int nu = (hidden + kValLanes - 1) / kValLanes;
  for (int64_t r = 0; r < n; ++r) {
    uint4 ra, rb;
    record_from_board(board + 24 * r, off[2 * r], off[2 * r + 1], 0u, 0u, player[r], 0u, 0u, ra, rb);
    uint2 root[kValRootSlots];
    const int nroot = val_root_list(ra, rb, ld, root);
    TdCols C;
    td_cols_of(ra, rb, C);
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
    const float val = val_out_act(b2[0] + part[0], out_act);
    const float go = val_out_slope(val, out_act);
    float d[kValHiddenMax], ga[kValHiddenMax];
    for (int h = 0; h < hidden; ++h) {
      const int t = h % kValLanes, i = h / kValLanes;
      td_unit_grad(go, w2t[t][i], z[t][i], a[t][i], hidden_act, ga[h], d[h]);
    }
    v[r] = val;
    black[r] = (uint8_t)((rb.z >> 10) & 1u);
    for (int c = 0; c < 198; ++c) cols[198 * r + c] = (C.mask[c >> 5] >> (c & 31)) & 1u;
    float* row = trace + r * ld_trace;
    for (int c = 0, p = 0; c <= kTdCols; ++c)
      for (int h = 0; h < (c < kTdCols ? hidden : 1); ++h, ++p) {
        float g = 0.0f;
        const bool hit = td_grad_at(c, h, C, d, ga, go, g);
        row[p] = td_trace_at(decay, decay != 0.0f ? row[p] : 0.0f, hit, g);
      }
  }
}

void hc_td_delta(int64_t n, const uint8_t* terminated, const uint8_t* truncated, const int32_t* reward,
                 const uint8_t* black, float gamma, const float* v_next, const float* v, float* delta) {
  for (int64_t e = 0; e < n; ++e)
    delta[e] = td_delta(terminated[e] != 0, truncated[e] != 0, reward[e], black[e], gamma, v_next[e], v[e]);
}

}  // extern "C"
