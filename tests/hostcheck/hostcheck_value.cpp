// hostcheck_value.cpp -- TEST-ONLY host build of the value-MLP arithmetic
// (gym-narde_amd/csrc/narde_rules.h "value MLP").
//
// Runs the functions the scored fill kernels (kernels_rows.h "the scored
// rows") run 16 lanes a row: the column lists of a record and of a row
// against its root, the per-hidden-unit accumulation, the activations and
// the lanes' sum, lane by lane in the wave's order.
// tests/test_value_cpu.py compares the lists with tes_value's rows bit for
// bit and the values with torch.  Never loaded by the product.
#include <cstring>

#include "../../gym-narde_amd/csrc/narde_rules.h"

using namespace narde;

namespace {

void record_of(const int8_t* board, const uint8_t* off, int8_t player, uint4& a, uint4& b) {
  record_from_board(board, off[0], off[1], 0u, 0u, player, 0u, 0u, a, b);
}

}  // namespace

extern "C" {

int hc_value_slots(void) { return kValRowSlots; }

// Per row r: its root (rboard i8[24] absolute, roff u8[2], rplayer i8) and
// itself (board, off, player).  Out: cnt i32 = tes_delta_walk's count, col
// i32[16], oldv / newv f32[16] its triples in order; feat_root / feat_row
// f32[198] = tes_value of the two records; nz_cnt i32, nz_col i32[48], nz_val
// f32[48] = the root's tes_item_nonzero entries, item by item.  Returns the largest count.
int hc_value_lists(int64_t n, const int8_t* rboard, const uint8_t* roff, const int8_t* rplayer, const int8_t* board,
                   const uint8_t* off, const int8_t* player, int32_t* cnt, int32_t* col, float* oldv, float* newv,
                   float* feat_root, float* feat_row, int32_t* nz_cnt, int32_t* nz_col, float* nz_val) {
  int most = 0;
  for (int64_t r = 0; r < n; ++r) {
    uint4 a0, b0, a1, b1;
    record_of(rboard + 24 * r, roff + 2 * r, rplayer[r], a0, b0);
    record_of(board + 24 * r, off + 2 * r, player[r], a1, b1);
    int k = 0;
    cnt[r] = tes_delta_walk(a0, b0, a1, b1, [&](int c, float o, float nw) {
      if (k < 16) {
        col[16 * r + k] = c;
        oldv[16 * r + k] = o;
        newv[16 * r + k] = nw;
      }
      ++k;
    });
    most = cnt[r] > most ? cnt[r] : most;
    for (int c = 0; c < 198; ++c) {
      feat_root[198 * r + c] = tes_value(a0, b0, c);
      feat_row[198 * r + c] = tes_value(a1, b1, c);
    }
    int q = 0;
    for (int item = 0; item < kValRootItems; ++item) {
      int c4[4];
      float v4[4];
      const int c = tes_item_nonzero(a0, b0, item, c4, v4);
      for (int j = 0; j < c; ++j, ++q)
        if (q < kValRootSlots) {
          nz_col[kValRootSlots * r + q] = c4[j];
          nz_val[kValRootSlots * r + q] = v4[j];
        }
    }
    nz_cnt[r] = q;
  }
  return most;
}

// value[r] as the scored fill writes it: rows as above, reward i8; the net
// w1t f32[198][ld], b1, w2 f32[hidden], b2 f32[1].  The 16 lanes of a row in
// turn, the record's own pre-activations in the four lane groups' parts, the
// lanes' parts summed in the wave's butterfly order.
void hc_value_rows(int64_t n, const int8_t* rboard, const uint8_t* roff, const int8_t* rplayer, const int8_t* board,
                   const uint8_t* off, const int8_t* player, const int8_t* reward, const float* w1t, int64_t ld,
                   const float* b1, const float* w2, const float* b2, int hidden, int hidden_act, int out_act,
                   int perspective, float* value) {
  uint4 pa{}, pb{};
  bool have = false;
  uint2 root[kValRootSlots];
  float zr[kValLanes][kValUnits] = {}, w2t[kValLanes][kValUnits];
  const int nu = (hidden + kValLanes - 1) / kValLanes;
  for (int t = 0; t < kValLanes; ++t)
    for (int i = 0; i < kValUnits; ++i) w2t[t][i] = t + kValLanes * i < hidden ? w2[t + kValLanes * i] : 0.0f;
  for (int64_t r = 0; r < n; ++r) {
    uint4 a0, b0, a1, b1r;
    record_of(rboard + 24 * r, roff + 2 * r, rplayer[r], a0, b0);
    record_of(board + 24 * r, off + 2 * r, player[r], a1, b1r);
    if (reward[r] != 0) {
      value[r] = val_outcome(reward[r], (b1r.z >> 10) & 1u, perspective);
      continue;
    }
    if (!have || memcmp(&pa, &a0, sizeof a0) || memcmp(&pb, &b0, sizeof b0)) {  // the env's part, once per env
      const int nroot = val_root_list(a0, b0, ld, root);
      for (int t = 0; t < kValLanes; ++t) {
        float p[kValRows][kValUnits];
        val_units(nu, [&](auto NU) {
          for (int g = 0; g < kValRows; ++g) val_root_part<NU.value>(root, nroot, g, w1t, t, hidden, p[g]);
        });
        for (int i = 0; i < nu; ++i)
          zr[t][i] = ((p[0][i] + p[1][i]) + (p[2][i] + p[3][i])) + (t + kValLanes * i < hidden ? b1[t + kValLanes * i] : 0.0f);
      }
      pa = a0;
      pb = b0;
      have = true;
    }
    uint2 list[kValRowSlots];
    const int cnt = val_row_list(a0, b0, a1, b1r, ld, list);
    float part[kValLanes], next[kValLanes];
    for (int t = 0; t < kValLanes; ++t) {
      float z[kValUnits];
      for (int i = 0; i < kValUnits; ++i) z[i] = zr[t][i];
      val_units(nu, [&](auto NU) {
        val_row_z<NU.value>(list, cnt > kValRowFirst, w1t, t, hidden, z);
        part[t] = val_lane_part<NU.value>(z, w2t[t], hidden_act);
      });
    }
    for (int o = kValLanes / 2; o > 0; o >>= 1) {
      for (int t = 0; t < kValLanes; ++t) next[t] = part[t] + part[t ^ o];
      memcpy(part, next, sizeof part);
    }
    value[r] = val_out_act(b2[0] + part[0], out_act);
  }
}

}  // extern "C"
