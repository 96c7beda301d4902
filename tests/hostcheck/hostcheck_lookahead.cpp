// hostcheck_lookahead.cpp -- TEST-ONLY host build of the two-ply lookahead
// (gym-narde_amd/csrc/kernels_lookahead.h).
//
// Runs serially the functions k_aft_fill_rec and k_aft_look run a lane per
// play and 16 lanes a reply: an env's rows (play_step_at, the expressibility
// test, play_key's dedupe, play_afterstate), each row's record as the root
// (val_root_list, val_root_part in the four lane groups' parts), and per
// ordered roll of the opponent the replies of that record, their column
// lists against it (val_row_list), their values lane by lane in the wave's
// order, the replier's best, for no reply what the step with the codes
// (0, 0) leaves (env_step), and the mean in double in roll order.
// tests/test_lookahead_cpu.py compares the result with a float64 pipeline
// over the C oracle.  Never loaded by the product.
#include <cstring>
#include <vector>

#include "../../gym-narde_amd/csrc/narde_rules.h"
#include "hostcheck_rows.h"

using namespace narde;

namespace {

struct Net {
  const float *w1t, *b1, *w2, *b2;
  int64_t ld;
  int hidden, hidden_act, out_act;
};

struct Root {
  uint4 a, b;
  float z[kValLanes][kValUnits];
  float w2t[kValLanes][kValUnits];
  int nu;
};

void root_of(const Net& n, const uint4& a, const uint4& b, Root& r) {
  r.a = a;
  r.b = b;
  r.nu = (n.hidden + kValLanes - 1) / kValLanes;
  uint2 list[kValRootSlots];
  const int nroot = val_root_list(a, b, n.ld, list);
  for (int t = 0; t < kValLanes; ++t) {
    float p[kValRows][kValUnits];
    val_units(r.nu, [&](auto NU) {
      for (int g = 0; g < kValRows; ++g) val_root_part<NU.value>(list, nroot, g, n.w1t, t, n.hidden, p[g]);
    });
    for (int i = 0; i < kValUnits; ++i) {
      const bool on = i < r.nu && t + kValLanes * i < n.hidden;
      r.z[t][i] = i < r.nu ? ((p[0][i] + p[1][i]) + (p[2][i] + p[3][i])) + (on ? n.b1[t + kValLanes * i] : 0.0f) : 0.0f;
      r.w2t[t][i] = on ? n.w2[t + kValLanes * i] : 0.0f;
    }
  }
}

// v(c) for a record c against its root, as val_rows_each gives it
float value_of(const Net& n, const Root& r, const uint4& ca, const uint4& cb) {
  uint2 list[kValRowSlots];
  const int cnt = val_row_list(r.a, r.b, ca, cb, n.ld, list);
  float part[kValLanes], next[kValLanes];
  for (int t = 0; t < kValLanes; ++t) {
    float z[kValUnits];
    for (int i = 0; i < kValUnits; ++i) z[i] = r.z[t][i];
    val_units(r.nu, [&](auto NU) {
      val_row_z<NU.value>(list, cnt > kValRowFirst, n.w1t, t, n.hidden, z);
      part[t] = val_lane_part<NU.value>(z, r.w2t[t], n.hidden_act);
    });
  }
  for (int o = kValLanes / 2; o > 0; o >>= 1) {
    for (int t = 0; t < kValLanes; ++t) next[t] = part[t] + part[t ^ o];
    memcpy(part, next, sizeof part);
  }
  return val_out_act(n.b2[0] + part[0], n.out_act);
}

// the kept plays of (s, d0, d1) in row order: visit(play)
template <typename F>
int kept_plays(const Side& s, int d0, int d1, F&& visit) {
  if (d0 < 1 || d0 > 6 || d1 < 1 || d1 > 6) return 0;
  Legal l;
  legal2(s, d0, d1, l);
  std::vector<uint32_t> keys;
  Play y;
  for (int j = 0; play_step_at(s, d0, d1, l, j, y); ++j) {
    if (!play_expressible(y, l.count == 1)) continue;
    const uint32_t key = play_key(y);
    bool seen = false;
    for (const uint32_t k : keys) seen = seen || k == key;
    if (seen) continue;
    keys.push_back(key);
    visit(y);
  }
  return (int)keys.size();
}

}  // namespace

extern "C" {

// narde_afterstates_lookahead on the host.  Envs as hc_afterstates (dice in
// roll order); dice_mode 0 all 36 ordered rolls, 1 the 30 unequal ones.
// Rows in CSR order, those below cap written: codes i16[2], reward i8, value
// f32, and for the test the row's record after the step -- rboard i8[24]
// (absolute), roff u8[2], rft u8[2], rplayer i8 -- and per ordered roll
// (a, b) at [row][6 (a - 1) + (b - 1)]: replies i16 = the number of reply
// rows (-1: a terminal row, or a roll the dice mode leaves out), terminal u8
// = 1 when one of them ends the game, best f32 = m(row, a, b).  Returns
// offsets[n].
int64_t hc_lookahead(int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft, const int8_t* player,
                     const uint8_t* dice, int64_t cap, int dice_mode, const float* w1t, int64_t ld, const float* b1,
                     const float* w2, const float* b2, int hidden, int hidden_act, int out_act, int32_t* offsets,
                     int16_t* codes, int8_t* reward, float* value, int8_t* rboard, uint8_t* roff, uint8_t* rft,
                     int8_t* rplayer, int16_t* replies, uint8_t* terminal, float* best) {
  const Net net{w1t, b1, w2, b2, ld, hidden, hidden_act, out_act};
  int64_t row = 0;
  offsets[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    const Side s = load_side(board + i * 24, off + 2 * i, ft + 2 * i, player[i]);
    kept_plays(s, dice[2 * i], dice[2 * i + 1], [&](const Play& y) {
      const int64_t R = row++;
      if (R >= cap) return;
      // k_aft_fill_rec: the narrow outputs, the record, a terminal row's outcome
      Side c = s;
      int term, rew, c1, c2;
      play_afterstate(c, y, term, rew);
      play_codes(y, c1, c2);
      codes[2 * R] = (int16_t)c1;
      codes[2 * R + 1] = (int16_t)c2;
      reward[R] = (int8_t)rew;
      uint4 ra, rb;
      side_to_record(c, ra, rb);
      board_from_record(ra, rb, rboard + 24 * R, roff + 2 * R, rft + 2 * R, rplayer + R, nullptr);
      for (int k = 0; k < 36; ++k) {
        replies[36 * R + k] = -1;
        terminal[36 * R + k] = 0;
        best[36 * R + k] = 0.0f;
      }
      if (rew != 0) {
        value[R] = val_outcome(rew, (rb.z >> 10) & 1u, 1);
        return;
      }
      // k_aft_look: the record is the root of every reply
      const Side sr = side_from_record(ra, rb);
      const bool smallest = sr.black != 0u;
      Root root;
      root_of(net, ra, rb, root);
      double sum = 0.0;
      int rolls = 0;
      for (int d0 = 1; d0 <= 6; ++d0)
        for (int d1 = 1; d1 <= 6; ++d1) {
          if (dice_mode == 1 && d0 == d1) continue;
          const int k = 6 * (d0 - 1) + (d1 - 1);
          float m = smallest ? __builtin_inff() : -__builtin_inff();
          const int cnt = kept_plays(sr, d0, d1, [&](const Play& z) {
            Side q = sr;
            int t2, r2;
            play_afterstate(q, z, t2, r2);
            uint4 ca, cb;
            side_to_record(q, ca, cb);
            const float v = r2 != 0 ? val_outcome(r2, (cb.z >> 10) & 1u, 1) : value_of(net, root, ca, cb);
            if (r2 != 0) terminal[36 * R + k] = 1;
            m = smallest ? fminf(m, v) : fmaxf(m, v);
          });
          if (cnt == 0) {  // what the step with the codes (0, 0) leaves
            Side q = sr;
            StepOut o;
            env_step(q, d0, d1, 0, 0, false, 0u, 0u, o);
            uint4 ca, cb;
            side_to_record(q, ca, cb);
            m = o.reward != 0 ? val_outcome(o.reward, (cb.z >> 10) & 1u, 1) : value_of(net, root, ca, cb);
          }
          replies[36 * R + k] = (int16_t)cnt;
          best[36 * R + k] = m;
          sum += (double)m;
          ++rolls;
        }
      value[R] = (float)(sum / (double)rolls);
    });
    offsets[i + 1] = (int32_t)row;
  }
  return row;
}

// env_step (what k_step runs) with the codes (0, 0) on n positions and
// their rolls; the position it leaves -> the same arrays, reward i8
void hc_lookahead_pass(int64_t n, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player, const uint8_t* dice,
                       int8_t* reward) {
  for (int64_t i = 0; i < n; ++i) {
    Side s = load_side(board + i * 24, off + 2 * i, ft + 2 * i, player[i]);
    StepOut o;
    env_step(s, dice[2 * i], dice[2 * i + 1], 0, 0, false, 0u, 0u, o);
    uint4 a, b;
    side_to_record(s, a, b);
    board_from_record(a, b, board + 24 * i, off + 2 * i, ft + 2 * i, player + i, nullptr);
    reward[i] = (int8_t)o.reward;
  }
}

}  // extern "C"
