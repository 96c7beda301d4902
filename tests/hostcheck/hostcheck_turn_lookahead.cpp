// hostcheck_turn_lookahead.cpp -- TEST-ONLY host build of the FULL4 two-ply
// lookahead (gym-narde_amd/csrc/kernels_turn_lookahead.h).
//
// Runs serially the functions k_turn_fill_rec, k_turn_look and
// k_turn_look_mean run a lane per node and 16 lanes a reply: an env's rows
// (the level walk: turn_root, turn_node_lists, turn_child, turn_path_key's
// dedupe; turn_path_apply, step_end), each row's record as the root
// (val_root_list, val_root_part in the four lane groups' parts), and per
// unordered roll a <= b of the opponent the level walk of that record, the
// final level's column lists against it (val_row_list), their values lane by
// lane in the wave's order, the replier's best, for a pass the record with
// the mover flipped (step_end), and the weighted mean in double in roll
// order.  tests/test_turn_lookahead_cpu.py compares the result with a
// float64 pipeline over the C oracle.  Never loaded by the product.
//
// The two host checks below are included whole for what they define: Net,
// Root, root_of, value_of (the scored forward against a root) and Node,
// turn_levels (the serial level walk).
#include "hostcheck_lookahead.cpp"
#include "hostcheck_turn_afterstates.cpp"

extern "C" {

// narde_turn_afterstates_lookahead on the host.  Envs as
// hc_turn_afterstates; dice_mode 0: all 21 unordered rolls (weight 1 a
// double, 2 otherwise), 1: the 15 unequal ones.  Rows in CSR order, those
// below cap written: play i8[4][2], reward i8, value f32, and for the test
// the row's record after the turn -- rboard i8[24] (absolute), roff u8[2],
// rft u8[2], rplayer i8 -- and per unordered roll k (a outer, b >= a inner)
// at [row][k]: replies i32 = the number of reply rows (-1: a terminal row,
// or a roll the dice mode leaves out; 0: a pass), front i32 = the reply
// walk's largest level, terminal u8 = 1 when a reply ends the game, best f32
// = m(row, roll).  Returns offsets[n].
int64_t hc_turn_lookahead(int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft, const int8_t* player,
                          const uint8_t* dice, int64_t cap, int dice_mode, const float* w1t, int64_t ld,
                          const float* b1, const float* w2, const float* b2, int hidden, int hidden_act, int out_act,
                          int32_t* offsets, int8_t* play, int8_t* reward, float* value, int8_t* rboard, uint8_t* roff,
                          uint8_t* rft, int8_t* rplayer, int32_t* replies, int32_t* front, uint8_t* terminal,
                          float* best) {
  const Net net{w1t, b1, w2, b2, ld, hidden, hidden_act, out_act};
  int64_t row = 0;
  offsets[0] = 0;
  std::vector<Node> rows, reps;
  for (int64_t i = 0; i < n; ++i) {
    const int d0 = dice[2 * i], d1 = dice[2 * i + 1];
    rows.clear();
    int M = 0, fr;
    const Side s = load_side(board + i * 24, off + 2 * i, ft + 2 * i, player[i]);
    if (d0 >= 1 && d0 <= 6 && d1 >= 1 && d1 <= 6) M = turn_levels(s, d0, d1, rows, fr);
    const int dh = d0 > d1 ? d0 : d1, dl = d0 > d1 ? d1 : d0;
    for (const Node& nd : rows) {
      const int64_t R = row++;
      if (R >= cap) continue;
      // k_turn_fill_rec: the narrow outputs, the record, a terminal row's outcome
      Side c = s;
      turn_path_apply(c, nd.path, M, dh, dl);
      int term, rew;
      step_end(c, false, term, rew);
      const uint64_t pw = turn_path_play(nd.path, M, dh, dl);
      memcpy(play + R * 8, &pw, 8);
      reward[R] = (int8_t)rew;
      uint4 ra, rb;
      side_to_record(c, ra, rb);
      board_from_record(ra, rb, rboard + 24 * R, roff + 2 * R, rft + 2 * R, rplayer + R, nullptr);
      for (int k = 0; k < 21; ++k) {
        replies[21 * R + k] = -1;
        front[21 * R + k] = 0;
        terminal[21 * R + k] = 0;
        best[21 * R + k] = 0.0f;
      }
      if (rew != 0) {
        value[R] = val_outcome(rew, (rb.z >> 10) & 1u, 1);
        continue;
      }
      // k_turn_look: the record is the root of every reply
      const Side sr = side_from_record(ra, rb);
      const bool smallest = sr.black != 0u;
      Root root;
      root_of(net, ra, rb, root);
      double sum = 0.0, weight = 0.0;
      int k = 0;
      for (int a = 1; a <= 6; ++a)
        for (int b = a; b <= 6; ++b, ++k) {
          if (dice_mode == 1 && a == b) continue;
          float m = smallest ? __builtin_inff() : -__builtin_inff();
          int f2;
          const int M2 = turn_levels(sr, a, b, reps, f2);
          for (const Node& rp : reps) {
            Side q = sr;
            turn_path_apply(q, rp.path, M2, b, a);
            int t2, r2;
            step_end(q, false, t2, r2);
            uint4 ca, cb;
            side_to_record(q, ca, cb);
            const float v = r2 != 0 ? val_outcome(r2, (cb.z >> 10) & 1u, 1) : value_of(net, root, ca, cb);
            if (r2 != 0) terminal[21 * R + k] = 1;
            m = smallest ? fminf(m, v) : fmaxf(m, v);
          }
          if (reps.empty()) {  // a pass: what the step with an all -1 play leaves
            Side q = sr;
            int t2, r2;
            step_end(q, false, t2, r2);
            uint4 ca, cb;
            side_to_record(q, ca, cb);
            m = r2 != 0 ? val_outcome(r2, (cb.z >> 10) & 1u, 1) : value_of(net, root, ca, cb);
          }
          replies[21 * R + k] = (int32_t)reps.size();
          front[21 * R + k] = f2;
          best[21 * R + k] = m;
          const double w = a == b ? 1.0 : 2.0;
          sum += w * (double)m;
          weight += w;
        }
      value[R] = (float)(sum / weight);
    }
    offsets[i + 1] = (int32_t)row;
  }
  return row;
}

}  // extern "C"
