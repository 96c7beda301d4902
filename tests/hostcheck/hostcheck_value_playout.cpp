// hostcheck_value_playout.cpp -- TEST-ONLY host build of the Monte-Carlo
// playouts (gym-narde_amd/csrc/kernels_value_playout.h and
// kernels_turn_value_playout.h), both rule sets.
//
// Runs serially, per trial and ply, the functions k_value_playout and
// k_turn_value_playout run a wave a trial: the root's record (record_from_board
// as narde_state_records packs it), the ply's words and dice on the call's own
// stream (ply_block with env id id_base + q, or id_base + j under common dice),
// the mover's net, the greedy row -- REF2: the kept plays' values against the
// record as root and RowBest's order, offered in the lanes the device holds
// them in and merged by the same butterfly; FULL4: the two-tier level walk
// (turn_levels_room) and the final level's rows the same way --, env_ply /
// env_ply_full with max_steps 0 and no auto-reset, the stop at the first
// terminal ply, the four integer sums and the leaf (the root forward and the
// second layer on the record the trial stopped at).  The roots, values and
// walks are hostcheck_lookahead.cpp's and hostcheck_turn_value_rollout.cpp's
// own functions, compiled in from those files.
// tests/test_value_playout_cpu.py compares the result with the host rollouts.
// Never loaded by the product.
#include "hostcheck_turn_value_rollout.cpp"

namespace {

// white's value of s under net: val_root's pre-activations, the second layer
float leaf_value(const Net& net, const Side& s) {
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  Root root;
  root_of(net, ra, rb, root);
  float part[kValLanes], next[kValLanes];
  for (int t = 0; t < kValLanes; ++t)
    val_units(root.nu, [&](auto NU) { part[t] = val_lane_part<NU.value>(root.z[t], root.w2t[t], net.hidden_act); });
  for (int o = kValLanes / 2; o > 0; o >>= 1) {
    for (int t = 0; t < kValLanes; ++t) next[t] = part[t] + part[t ^ o];
    memcpy(part, next, sizeof part);
  }
  return val_out_act(net.b2[0] + part[0], net.out_act);
}

RowBest merged(RowBest (&lanes)[64]) {
  for (int o = 32; o > 0; o >>= 1) {
    RowBest next[64];
    for (int q = 0; q < 64; ++q) {
      next[q] = lanes[q];
      row_best_merge(next[q], lanes[q ^ o]);
    }
    memcpy(lanes, next, sizeof lanes);
  }
  return lanes[0];
}

// REF2: the greedy row of (s, d0, d1) under net (vr_choose, want_explore false)
RowBest ref2_best(const Side& s, int d0, int d1, const Net& net) {
  const bool smallest = s.black != 0u;
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  Root root;
  root_of(net, ra, rb, root);
  RowBest lanes[64];
  for (int q = 0; q < 64; ++q) lanes[q] = row_best_none();
  int ord = 0;
  kept_plays(s, d0, d1, [&](const Play& y) {
    const int o = ord++;
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
  return merged(lanes);
}

// FULL4: the play word of the greedy row of (s, d0, d1) under net
// (turn_pick_roll on the chip tier, then in the slab; turn_pick_level): the
// all -1 play when the roll has no row
uint64_t full4_best(const Side& s, int d0, int d1, const Net& net, int room, std::vector<Node>& level) {
  int fr = 0;
  int M = turn_levels_room(s, d0, d1, room, level, fr);
  if (M < 0) M = turn_levels_room(s, d0, d1, kTurnAftMax, level, fr);
  const int count = M < 0 ? 0 : (int)level.size();
  if (count <= 0) return ~0ull;
  const bool smallest = s.black != 0u;
  const int dh = d0 > d1 ? d0 : d1, dl = d0 > d1 ? d1 : d0;
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  Root root;
  root_of(net, ra, rb, root);
  RowBest lanes[64];
  for (int q = 0; q < 64; ++q) lanes[q] = row_best_none();
  for (int g = 0; g < count; ++g) {
    const int q = g & 63;
    const uint32_t path = level[g].path;
    Side c = s;
    turn_path_apply(c, path, M, dh, dl);
    int tm, rew;
    step_end(c, false, tm, rew);
    uint4 ca, cb;
    side_to_record(c, ca, cb);
    if (rew != 0)
      row_best_offer(lanes[q], val_outcome(rew, (cb.z >> 10) & 1u, 1), g, path, smallest);
    else
      row_best_offer(lanes[kValLanes * (q % kValRows)], value_of(net, root, ca, cb), g, path, smallest);
  }
  const RowBest best = merged(lanes);
  return turn_path_play_words(best.codes, M, dh, dl);
}

}  // namespace

extern "C" {

// narde_value_playout (full 0) / narde_turn_value_playout (full 1; `room` the
// walk's first tier) on the host: n roots (board, off, ft, player; ply counter
// t, elapsed 0), trials each.  Outputs: records u32[n][8] (narde_state_records'
// packing), sums i32[n][4], outcome i8[n][trials], length i32[n][trials], leaf
// f32[n][trials].
void hc_value_playout(int full, int room, int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft,
                      const int8_t* player, uint32_t t, int trials, int max_plies, const NetIn* white,
                      const NetIn* black, uint64_t seed, int64_t id_base, int common, int dice_mode, uint32_t* records,
                      int32_t* sums, int8_t* outcome, int32_t* length, float* leaf) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  std::vector<Node> level;
  for (int64_t i = 0; i < n; ++i) {
    uint4 a, b;
    record_from_board(board + i * 24, off[2 * i], off[2 * i + 1], ft[2 * i], ft[2 * i + 1], player[i], 0u, t, a, b);
    memcpy(records + 8 * i, &a, 16);
    memcpy(records + 8 * i + 4, &b, 16);
    for (int l = 0; l < 4; ++l) sums[4 * i + l] = 0;
    for (int j = 0; j < trials; ++j) {
      const int64_t q = i * trials + j;
      const uint32_t env = (uint32_t)(id_base + (common ? j : q));
      Side s = side_from_record(a, b);
      int done = 0, outc = 0, len = 0;
      uint32_t R[4];
      for (int k = 0; k < max_plies; ++k) {
        uint32_t r[4];
        if (k == 0 || (s.t & 1u) == 0u) ply_block(s.t, env, k0, k1, R);
        ply_words_of(R, s.t, dice_mode, r);
        int d0, d1;
        dice_from(r[0], dice_mode, d0, d1);
        const bool mover_black = s.black != 0u;
        const NetIn& in = mover_black ? *black : *white;
        const bool has = in.hidden > 0;
        const Net net{in.w1t, in.b1, in.w2, in.b2, in.ld, in.hidden, in.hidden_act, in.out_act};
        int4 st = make_int4(0, 0, 0, 0);
        int tm, tr, rew;
        if (full) {
          const uint64_t pw = has ? full4_best(s, d0, d1, net, room, level) : ~0ull;
          TurnOut o;
          env_ply_full(s, st, r, env, k0, k1, false, 0, 0, dice_mode, has, pw, 0, false, o, tm, tr);
          rew = o.reward;
        } else {
          const RowBest best = has ? ref2_best(s, d0, d1, net) : row_best_none();
          const int c1 = (int)(int16_t)(best.codes & 0xFFFFu), c2 = (int)(int16_t)(best.codes >> 16);
          StepOut o;
          env_ply(s, st, r, false, 0, 0, dice_mode, !has, c1, c2, 0, false, o, tm, tr);
          rew = o.reward;
        }
        len = k + 1;
        if (tm) {
          done = 1;
          outc = mover_black ? -rew : rew;
          break;
        }
      }
      float lv = __builtin_nanf("");
      if (!done) {
        const bool use_b = s.black ? black->hidden > 0 : white->hidden == 0;
        const NetIn& in = use_b ? *black : *white;
        lv = leaf_value(Net{in.w1t, in.b1, in.w2, in.b2, in.ld, in.hidden, in.hidden_act, in.out_act}, s);
      }
      outcome[q] = (int8_t)outc;
      length[q] = len;
      leaf[q] = lv;
      sums[4 * i] += done;
      sums[4 * i + 1] += outc;
      sums[4 * i + 2] += outc * outc;
      sums[4 * i + 3] += len;
    }
  }
}

}  // extern "C"
