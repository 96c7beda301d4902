// hostcheck_turn_value_rollout.cpp -- TEST-ONLY host build of the FULL4 value
// rollout (gym-narde_amd/csrc/kernels_turn_value_rollout.h).
//
// Runs serially, per env and ply, the functions k_turn_value_rollout runs a
// wave an env: the ply's words and dice (ply_block, ply_words_of, dice_from),
// the mover's net, the explore draw (explore_draw), the roll's level walk on
// the env's own record with `room` nodes a level and, when a level outgrows
// that, again with kTurnAftMax (the two tiers; turn_root, turn_node_lists,
// turn_child, turn_path_key's dedupe), the final level's rows (turn_path_apply,
// step_end), their values against the record as root lane by lane in the
// wave's order, the best row by RowBest's order (row_best_offer /
// row_best_merge: offered in the lanes that hold them on the device -- a
// terminal row from its node's lane, a scored row from its lane group's first
// lane -- and merged by the same butterfly) with the path word as payload,
// turn_path_play_words, and env_ply_full with that play word or, for a colour with
// no net, the random-legal policy.  The roots, values and the serial walk are
// hostcheck_turn_lookahead.cpp's, compiled in from that file.
// tests/test_turn_value_rollout_cpu.py replays the result over the C oracle.
// Never loaded by the product.
#include "hostcheck_turn_lookahead.cpp"

namespace {

struct NetIn {
  const float *w1t, *b1, *w2, *b2;
  int64_t ld;
  int32_t hidden, hidden_act, out_act;  // hidden 0: no net, the colour plays the random-legal policy
};

// turn_levels with the device walk's bound: -1 (nothing kept) as soon as a
// level holds more than `room` nodes; else M.  front: the largest level met.
int turn_levels_room(const Side& s, int d0, int d1, int room, std::vector<Node>& rows, int& front) {
  const TurnRoot r = turn_root(s, d0, d1);
  std::vector<Node> cur{{kTurnNoPath, 0ull}}, nxt;
  int level = 0, nh1 = 0;
  front = 0;
  rows.clear();
  for (; level < r.depth; ++level) {
    nxt.clear();
    for (const Node& nd : cur) {
      Side c = s;
      turn_path_apply(c, nd.path, level, r.dh, r.dl);
      uint32_t w0, w1;
      turn_node_lists(c, nd.path, level, r, w0, w1);
      if (level == 0) nh1 = __builtin_popcount(w0 & MASK24);
      const int cnt = __builtin_popcount(w0 & MASK24) + __builtin_popcount(w1 & MASK24);
      for (int j = 0; j < cnt; ++j) {
        const uint32_t cp = turn_child(nd.path, level, w0, w1, j);
        const uint64_t key = turn_path_key(cp, level + 1, r.dh, r.dl, r.dh != r.dl && level == 0);
        bool seen = false;
        for (const Node& o : nxt) seen = seen || o.key == key;
        if (seen) continue;
        if ((int)nxt.size() + 1 > room) return -1;
        nxt.push_back({cp, key});
      }
    }
    if (nxt.empty()) break;
    cur.swap(nxt);
    front = (int)cur.size() > front ? (int)cur.size() : front;
  }
  if (level == 0) return 0;
  rows = cur;
  if (r.dh != r.dl && level == 1 && nh1 > 0) rows.resize(nh1);
  return level;
}

}  // namespace

extern "C" {

int hc_turn_rollout_piece() { return (int)((kTurnAftMax + 2) * sizeof(uint64_t) + 2 * kTurnAftMax * sizeof(uint32_t)); }

// narde_turn_value_rollout on the host: n envs from (board, off, ft, player,
// elapsed, t) -- updated in place, stats i32[n][3] added to -- for `plies`
// plies, the walk's first tier `room` nodes a level.  Outputs [plies][n]:
// dice u8[2], play i8[4][2], value f32, reward i32, term u8, trunc u8, and for
// the test words u32[4] (the ply's words), rows i32 (the roll's row count, -1
// on a random ply), row i32 (the ordinal played, -1 for none), explored u8,
// tier u8 (1: the walk outgrew `room` and ran again at kTurnAftMax), front i32
// (the walk's largest level), mdice i32 (the turn's max_dice as the step
// reports it).
void hc_turn_value_rollout(int64_t n, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player, uint16_t* elapsed,
                           uint32_t* t, int32_t* stats, int64_t env0, uint64_t seed, int dice_mode, int max_steps,
                           int plies, int room, const NetIn* white, const NetIn* black, int use_eps, float eps,
                           uint64_t pick_seed, int64_t tag, uint8_t* dice, int8_t* play, float* value, int32_t* reward,
                           uint8_t* term, uint8_t* trunc, uint32_t* words, int32_t* rows, int32_t* row,
                           uint8_t* explored, uint8_t* tier, int32_t* front, int32_t* mdice) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t p0 = (uint32_t)pick_seed, p1 = (uint32_t)(pick_seed >> 32);
  const uint64_t eps_q32 = use_eps ? eps_to_q32(eps) : 0ull;
  std::vector<Node> level;
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
      uint64_t pw = ~0ull;
      int count = -1, fr = 0;
      bool explore = false, second = false;
      if (has) {
        const Net net{in.w1t, in.b1, in.w2, in.b2, in.ld, in.hidden, in.hidden_act, in.out_act};
        uint32_t r1 = 0u;
        explore = use_eps && explore_draw((uint32_t)(tag + k), (uint32_t)e, p0, p1, eps_q32, r1);
        const bool smallest = s.black != 0u;
        int M = turn_levels_room(s, d0, d1, room, level, fr);
        if (M < 0) {
          second = true;
          M = turn_levels_room(s, d0, d1, kTurnAftMax, level, fr);
        }
        count = M < 0 ? 0 : (int)level.size();
        if (count > 0) {
          const int dh = d0 > d1 ? d0 : d1, dl = d0 > d1 ? d1 : d0;
          uint4 ra, rb;
          side_to_record(s, ra, rb);
          Root root;
          root_of(net, ra, rb, root);
          const int want = explore ? (int)mulhi_u32(r1, (uint32_t)count) : -1;
          RowBest lanes[64];
          for (int q = 0; q < 64; ++q) lanes[q] = row_best_none();
          const int g1 = want < 0 ? count : want + 1;
          for (int g0 = want < 0 ? 0 : want; g0 < g1; g0 += 64) {
            const int nr = g1 - g0 < 64 ? g1 - g0 : 64;
            for (int q = 0; q < nr; ++q) {
              const uint32_t path = level[g0 + q].path;
              Side c = s;
              turn_path_apply(c, path, M, dh, dl);
              int tm, rew;
              step_end(c, false, tm, rew);
              uint4 ca, cb;
              side_to_record(c, ca, cb);
              if (rew != 0)
                row_best_offer(lanes[q], val_outcome(rew, (cb.z >> 10) & 1u, 1), g0 + q, path, smallest);
              else
                row_best_offer(lanes[kValLanes * (q % kValRows)], value_of(net, root, ca, cb), g0 + q, path, smallest);
            }
          }
          for (int o = 32; o > 0; o >>= 1) {
            RowBest next[64];
            for (int q = 0; q < 64; ++q) {
              next[q] = lanes[q];
              row_best_merge(next[q], lanes[q ^ o]);
            }
            memcpy(lanes, next, sizeof lanes);
          }
          best = lanes[0];
          pw = turn_path_play_words(best.codes, M, dh, dl);
        }
      }
      TurnOut o;
      int tm, tr;
      env_ply_full(s, st, r, (uint32_t)(env0 + e), k0, k1, false, 0, 0, dice_mode, has, pw, max_steps, true, o, tm,
                   tr);
      const uint64_t pl = has ? pw : o.played;
      dice[2 * ix] = (uint8_t)d0;
      dice[2 * ix + 1] = (uint8_t)d1;
      memcpy(play + 8 * ix, &pl, 8);
      value[ix] = best.ord >= 0 ? best.v : __builtin_nanf("");
      reward[ix] = o.reward;
      term[ix] = (uint8_t)tm;
      trunc[ix] = (uint8_t)tr;
      for (int j = 0; j < 4; ++j) words[4 * ix + j] = r[j];
      rows[ix] = count;
      row[ix] = best.ord;
      explored[ix] = explore ? 1 : 0;
      tier[ix] = second ? 1 : 0;
      front[ix] = fr;
      mdice[ix] = o.max_dice;
    }
    side_to_record(s, a, b);
    board_from_record(a, b, board + e * 24, off + 2 * e, ft + 2 * e, player + e, elapsed + e);
    t[e] = s.t;
    stats[3 * e] += st.x;
    stats[3 * e + 1] += st.y;
    stats[3 * e + 2] += st.z;
  }
}

// narde_step_full(play = NULL, dice = NULL, autoreset = 1) on the host, one
// ply of n envs in place (env_ply_full, play = false): what a colour with no
// net must equal.  Outputs [n]: played i8[4][2], reward i32, term u8, trunc u8.
void hc_turn_random_ply(int64_t n, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player, uint16_t* elapsed,
                        uint32_t* t, int32_t* stats, int64_t env0, uint64_t seed, int dice_mode, int max_steps,
                        int8_t* played, int32_t* reward, uint8_t* term, uint8_t* trunc) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t e = 0; e < n; ++e) {
    uint4 a, b;
    record_from_board(board + e * 24, off[2 * e], off[2 * e + 1], ft[2 * e], ft[2 * e + 1], player[e], elapsed[e],
                      t[e], a, b);
    Side s = side_from_record(a, b);
    int4 st = make_int4(0, 0, 0, 0);
    uint32_t R[4], r[4];
    ply_block(s.t, (uint32_t)(env0 + e), k0, k1, R);
    ply_words_of(R, s.t, dice_mode, r);
    TurnOut o;
    int tm, tr;
    env_ply_full(s, st, r, (uint32_t)(env0 + e), k0, k1, false, 0, 0, dice_mode, false, 0ull, max_steps, true, o, tm,
                 tr);
    memcpy(played + 8 * e, &o.played, 8);
    reward[e] = o.reward;
    term[e] = (uint8_t)tm;
    trunc[e] = (uint8_t)tr;
    side_to_record(s, a, b);
    board_from_record(a, b, board + e * 24, off + 2 * e, ft + 2 * e, player + e, elapsed + e);
    t[e] = s.t;
    stats[3 * e] += st.x;
    stats[3 * e + 1] += st.y;
    stats[3 * e + 2] += st.z;
  }
}

}  // extern "C"
