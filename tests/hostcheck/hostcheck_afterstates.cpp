// hostcheck_afterstates.cpp -- TEST-ONLY host build of the afterstate rules
// layer (gym-narde_amd/csrc/narde_rules.h "afterstates").
//
// Walks each env's plays serially through the functions the kernels
// (kernels_afterstates.h) run a lane per play: play_step_at, the
// expressibility test, play_key's dedupe, play_afterstate, play_codes, and
// the 198-float row by tes_value.  tests/test_afterstates_cpu.py compares
// the ordered rows with a restatement over the C oracle.  Never loaded by
// the product.
#include <cstring>
#include <vector>

#include "../../gym-narde_amd/csrc/narde_rules.h"
#include "hostcheck_rows.h"

using namespace narde;

extern "C" {

// Rows in CSR order: env i's rows are offsets[i] .. offsets[i + 1] - 1 (true
// counts); rows below cap are written: codes i16[2], board i8[24] (absolute),
// off u8[2], player i8 (after the step), reward i8, feat f32[198].  plays[i]
// = play_walk's kPlayStep count (0 for a die outside 1..6).  dice in roll
// order.  Returns offsets[n].
int64_t hc_afterstates(int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft, const int8_t* player,
                       const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* plays, int16_t* codes,
                       int8_t* boards, uint8_t* offs, int8_t* players, int8_t* reward, float* feat) {
  int64_t row = 0;
  offsets[0] = 0;
  std::vector<uint32_t> keys;
  for (int64_t i = 0; i < n; ++i) {
    const int d0 = dice[2 * i], d1 = dice[2 * i + 1];
    plays[i] = 0;
    if (d0 >= 1 && d0 <= 6 && d1 >= 1 && d1 <= 6) {
      const Side s = load_side(board + i * 24, off + 2 * i, ft + 2 * i, player[i]);
      Legal l;
      legal2(s, d0, d1, l);
      plays[i] = play_walk(s, d0, d1, kPlayStep, l, [](int, int, int, uint32_t, bool) {});
      keys.clear();
      Play y;
      for (int j = 0; play_step_at(s, d0, d1, l, j, y); ++j) {
        if (!play_expressible(y, l.count == 1)) continue;
        const uint32_t key = play_key(y);
        bool seen = false;
        for (const uint32_t k : keys) seen = seen || k == key;
        if (seen) continue;
        keys.push_back(key);
        if (row < cap) {
          Side c = s;
          int term, rew, c1, c2;
          play_afterstate(c, y, term, rew);
          play_codes(y, c1, c2);
          codes[2 * row] = (int16_t)c1;
          codes[2 * row + 1] = (int16_t)c2;
          write_row(c, rew, row, boards, offs, players, reward, feat);
        }
        ++row;
      }
    }
    offsets[i + 1] = (int32_t)row;
  }
  return row;
}

// play_key against board + off identity on every pair of env 0's plays (the
// expressible flag ignored): returns the number of pairs on which the two
// disagree
int64_t hc_afterstate_key_pairs(const int8_t* board, const uint8_t* off, const uint8_t* ft, int8_t player,
                                const uint8_t* dice) {
  const Side s = load_side(board, off, ft, player);
  Legal l;
  legal2(s, dice[0], dice[1], l);
  std::vector<uint32_t> keys;
  std::vector<uint4> recs;
  Play y;
  for (int j = 0; play_step_at(s, dice[0], dice[1], l, j, y); ++j) {
    Side c = s;
    int term, rew;
    play_afterstate(c, y, term, rew);
    uint4 ra, rb;
    side_to_record(c, ra, rb);
    keys.push_back(play_key(y));
    recs.push_back(ra);
    recs.push_back(rb);
  }
  int64_t bad = 0;
  for (size_t p = 0; p < keys.size(); ++p)
    for (size_t q = 0; q < p; ++q) {
      const bool same = memcmp(&recs[2 * p], &recs[2 * q], 2 * sizeof(uint4)) == 0;
      bad += same != (keys[p] == keys[q]);
    }
  return bad;
}

}  // extern "C"
