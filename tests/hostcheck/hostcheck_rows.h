// hostcheck_rows.h -- TEST-ONLY: what the two afterstate host checks
// (hostcheck_afterstates.cpp, hostcheck_turn_afterstates.cpp) share: a
// position's Side from the test's arrays, and one afterstate row written to
// them.  Included behind narde_rules.h.
#pragma once

namespace {

using namespace narde;

Side load_side(const int8_t* board, const uint8_t* off, const uint8_t* ft, int8_t player) {
  uint4 a, b;
  record_from_board(board, off[0], off[1], ft[0], ft[1], player, 0u, 0u, a, b);
  return side_from_record(a, b);
}

// row `row` of the afterstate c: board i8[24] (absolute), off u8[2], player
// i8, reward i8, feat f32[198] (tes_value)
void write_row(const Side& c, int rew, int64_t row, int8_t* boards, uint8_t* offs, int8_t* players, int8_t* reward,
               float* feat) {
  uint4 ra, rb;
  side_to_record(c, ra, rb);
  board_from_record(ra, rb, boards + row * 24, offs + 2 * row, nullptr, players + row, nullptr);
  reward[row] = (int8_t)rew;
  for (int col = 0; col < 198; ++col) feat[row * 198 + col] = tes_value(ra, rb, col);
}

}  // namespace
