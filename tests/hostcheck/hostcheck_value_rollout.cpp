// hostcheck_value_rollout.cpp -- TEST-ONLY host build of the value rollout
// (gym-narde_amd/csrc/kernels_value_rollout.h).
//
// Runs serially, per env and ply, the functions k_value_rollout runs a wave
// an env: the ply's words and dice (ply_block, ply_words_of, dice_from), the
// mover's net, the explore draw (explore_draw), the roll's rows on the env's
// own record (the kept plays, play_afterstate, play_codes), their values
// against the record as root lane by lane in the wave's order, the best row
// by RowBest's order (row_best_offer / row_best_merge: offered here in the
// order the wave's lanes hold them -- terminal rows from the play's lane,
// scored rows from their lane group's first lane -- and merged by the same
// butterfly), and env_ply with the row's codes or, for a colour with no net,
// the random-legal policy.  The rows, roots and values are
// hostcheck_lookahead.cpp's own functions, compiled in from that file.
// tests/test_value_rollout_cpu.py replays the result over the C oracle.
// Never loaded by the product.
#include "hostcheck_lookahead.cpp"

namespace {

struct NetIn {
  const float *w1t, *b1, *w2, *b2;
  int64_t ld;
  int32_t hidden, hidden_act, out_act;  // hidden 0: no net, the colour plays the random-legal policy
};

}  // namespace

extern "C" {

// narde_value_rollout on the host: n envs from (board, off, ft, player,
// elapsed, t) -- updated in place, stats i32[n][3] added to -- for `plies`
// plies.  Outputs [plies][n]: dice u8[2], actions i16[2], value f32, reward
// i32, term u8, trunc u8, and for the test words u32[4] (the ply's words),
// rows i32 (the roll's row count, -1 on a random ply), row i32 (the ordinal
// played, -1 for none), explored u8.
void hc_value_rollout(int64_t n, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player, uint16_t* elapsed,
                      uint32_t* t, int32_t* stats, int64_t env0, uint64_t seed, int dice_mode, int max_steps, int plies,
                      const NetIn* white, const NetIn* black, int use_eps, float eps, uint64_t pick_seed, int64_t tag,
                      uint8_t* dice, int16_t* actions, float* value, int32_t* reward, uint8_t* term, uint8_t* trunc,
                      uint32_t* words, int32_t* rows, int32_t* row, uint8_t* explored) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t p0 = (uint32_t)pick_seed, p1 = (uint32_t)(pick_seed >> 32);
  const uint64_t eps_q32 = use_eps ? eps_to_q32(eps) : 0ull;
  for (int64_t e = 0; e < n; ++e) {
    uint4 a, b;
    record_from_board(board + e * 24, off[2 * e], off[2 * e + 1], ft[2 * e], ft[2 * e + 1], player[e], elapsed[e],
                      t[e], a, b);
    Side s = side_from_record(a, b);
    int4 st = make_int4(0, 0, 0, 0);
    uint32_t R[4];
    for (int k = 0; k < plies; ++k) {
      const int64_t ix = (int64_t)k * n + e;
      uint32_t r[4];
      if (k == 0 || (s.t & 1u) == 0u) ply_block(s.t, (uint32_t)(env0 + e), k0, k1, R);
      ply_words_of(R, s.t, dice_mode, r);
      int d0, d1;
      dice_from(r[0], dice_mode, d0, d1);
      const NetIn& in = s.black ? *black : *white;
      const bool has = in.hidden > 0;
      RowBest best = row_best_none();
      int count = -1;
      bool explore = false;
      if (has) {
        const Net net{in.w1t, in.b1, in.w2, in.b2, in.ld, in.hidden, in.hidden_act, in.out_act};
        uint32_t r1 = 0u;
        explore = use_eps && explore_draw((uint32_t)(tag + k), (uint32_t)e, p0, p1, eps_q32, r1);
        const bool smallest = s.black != 0u;
        int want = -1;
        if (explore) {
          count = kept_plays(s, d0, d1, [](const Play&) {});
          if (count > 0) want = (int)mulhi_u32(r1, (uint32_t)count);
        }
        if (!explore || count > 0) {
          uint4 ra, rb;
          side_to_record(s, ra, rb);
          Root root;
          root_of(net, ra, rb, root);
          // a lane's best so far: a chunk's terminal row of rank q is offered by
          // the lane of its play, its scored row by lane 16 (q % 4); the wave's
          // play lanes are not known here, so terminal rows go to lane 63 - q % 64
          // -- the order is total, whichever lane holds a candidate
          RowBest lanes[64];
          for (int q = 0; q < 64; ++q) lanes[q] = row_best_none();
          int ord = 0;
          count = kept_plays(s, d0, d1, [&](const Play& y) {
            const int o = ord++;
            if (want >= 0 && o != want) return;
            Side c = s;
            int tm, rew, c1, c2;
            play_afterstate(c, y, tm, rew);
            play_codes(y, c1, c2);
            uint4 ca, cb;
            side_to_record(c, ca, cb);
            const uint32_t pk = pack_codes(c1, c2);
            if (rew != 0)
              row_best_offer(lanes[63 - (o & 63)], val_outcome(rew, (cb.z >> 10) & 1u, 1), o, pk, smallest);
            else
              row_best_offer(lanes[kValLanes * (o % kValRows)], value_of(net, root, ca, cb), o, pk, smallest);
          });
          for (int o = 32; o > 0; o >>= 1) {
            RowBest next[64];
            for (int q = 0; q < 64; ++q) {
              next[q] = lanes[q];
              row_best_merge(next[q], lanes[q ^ o]);
            }
            memcpy(lanes, next, sizeof lanes);
          }
          best = lanes[0];
        }
      }
      const int c1 = (int)(int16_t)(best.codes & 0xFFFFu), c2 = (int)(int16_t)(best.codes >> 16);
      StepOut o;
      int tm, tr;
      env_ply(s, st, r, false, 0, 0, dice_mode, !has, c1, c2, max_steps, true, o, tm, tr);
      dice[2 * ix] = (uint8_t)d0;
      dice[2 * ix + 1] = (uint8_t)d1;
      actions[2 * ix] = (int16_t)o.code1;
      actions[2 * ix + 1] = (int16_t)o.code2;
      value[ix] = best.ord >= 0 ? best.v : __builtin_nanf("");
      reward[ix] = o.reward;
      term[ix] = (uint8_t)tm;
      trunc[ix] = (uint8_t)tr;
      for (int j = 0; j < 4; ++j) words[4 * ix + j] = r[j];
      rows[ix] = count;
      row[ix] = best.ord;
      explored[ix] = explore ? 1 : 0;
    }
    side_to_record(s, a, b);
    board_from_record(a, b, board + e * 24, off + 2 * e, ft + 2 * e, player + e, elapsed + e);
    t[e] = s.t;
    stats[3 * e] += st.x;
    stats[3 * e + 1] += st.y;
    stats[3 * e + 2] += st.z;
  }
}

}  // extern "C"
