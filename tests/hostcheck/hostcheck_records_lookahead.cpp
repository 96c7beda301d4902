// hostcheck_records_lookahead.cpp -- TEST-ONLY host build of the two-ply
// values of given records and the pick over given slot scores
// (narde_records_lookahead, narde_turn_records_lookahead, narde_slot_pick;
// DESIGN.md section 25), both rule sets.
//
// Runs serially, on a caller's public records, the functions the look
// kernels' second instantiations run: the finished test (record_finished),
// the record as the root of every reply (root_of), per roll of the record's
// mover the replies -- REF2: kept_plays, play_afterstate, for no reply what
// env_step with the codes (0, 0) leaves; FULL4: the serial level walk
// (turn_levels), turn_path_apply, step_end, for a pass the record with the
// mover flipped --, their values against the root (value_of), the mover's
// best, and the mean in the kernels' order: in double, rounded once.  Word 7
// of a record is never read.  The slot pick is the device's own function
// (slot_pick_slot).  The rows, roots and values are hostcheck_lookahead.cpp's
// and hostcheck_turn_afterstates.cpp's own functions, compiled in through
// hostcheck_turn_lookahead.cpp, whose hc_lookahead and hc_turn_lookahead this
// library exports as well.  tests/test_records_lookahead_cpu.py compares the
// results with those two and with float64 pipelines over the C oracle.  Never
// loaded by the product.
#include "hostcheck_turn_lookahead.cpp"

extern "C" {

// record_from_board on n positions: records u32[n][8] with the given elapsed
// (u16[n] or NULL: 0) and ply counter words (u32[n] or NULL: 0)
void hc_pack_records(int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft, const int8_t* player,
                     const uint16_t* elapsed, const uint32_t* t, uint32_t* records) {
  for (int64_t i = 0; i < n; ++i) {
    uint4 a, b;
    record_from_board(board + 24 * i, off[2 * i], off[2 * i + 1], ft[2 * i], ft[2 * i + 1], player[i],
                      elapsed ? elapsed[i] : 0u, t ? t[i] : 0u, a, b);
    memcpy(records + 8 * i, &a, 16);
    memcpy(records + 8 * i + 4, &b, 16);
  }
}

// narde_records_lookahead (full 0) / narde_turn_records_lookahead (full 1) on
// the host: value f32[n]; for the test, per record and roll -- REF2 at
// [i][6 (a - 1) + (b - 1)] of 36, FULL4 at [i][k] of 21, k over a <= b, a
// outer -- replies i32 = the number of reply rows (-1: a finished record, or a
// roll the dice mode leaves out), front i32 = the reply walk's largest level
// (FULL4; 0 for REF2), best f32 = the roll's m.
void hc_records_lookahead(int full, int64_t n, const uint32_t* records, int dice_mode, const float* w1t, int64_t ld,
                          const float* b1, const float* w2, const float* b2, int hidden, int hidden_act, int out_act,
                          float* value, int32_t* replies, int32_t* front, float* best) {
  const Net net{w1t, b1, w2, b2, ld, hidden, hidden_act, out_act};
  const int per = full ? 21 : 36;
  std::vector<Node> reps;
  for (int64_t i = 0; i < n; ++i) {
    uint4 ra, rb;
    memcpy(&ra, records + 8 * i, 16);
    memcpy(&rb, records + 8 * i + 4, 16);
    for (int k = 0; k < per; ++k) {
      replies[per * i + k] = -1;
      front[per * i + k] = 0;
      best[per * i + k] = 0.0f;
    }
    if (record_finished(rb.z)) {
      value[i] = __builtin_nanf("");
      continue;
    }
    const Side sr = side_from_record(ra, rb);
    const bool smallest = sr.black != 0u;
    Root root;
    root_of(net, ra, rb, root);
    double sum = 0.0, weight = 0.0;
    if (!full) {  // k_aft_look: the 36 (30) ordered rolls, a outer, b inner
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
          replies[per * i + k] = cnt;
          best[per * i + k] = m;
          sum += (double)m;
          weight += 1.0;
        }
    } else {  // k_turn_look, k_turn_look_mean: the 21 (15) unordered rolls, 1 a double and 2 otherwise
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
          replies[per * i + k] = (int32_t)reps.size();
          front[per * i + k] = f2;
          best[per * i + k] = m;
          const double w = a == b ? 1.0 : 2.0;
          sum += w * (double)m;
          weight += w;
        }
    }
    value[i] = (float)(sum / weight);
  }
}

// narde_slot_pick / narde_turn_slot_pick on the host: words of `word` bytes
// (4: the two codes, no row 0; 8: the play, no row -1) from column to out;
// black u8[n] = the env's mover is black
void hc_slot_pick(int64_t n, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld,
                  const int8_t* reward, const void* column, int word, const float* slot_score, const uint8_t* black,
                  void* out, int32_t* row, float* score) {
  for (int64_t e = 0; e < n; ++e) {
    const int64_t s0 = e * k;
    const int b = slot_pick_slot(sel + s0, k, cap, value, ld, reward, slot_score + s0, black[e] != 0, score + s0);
    const int64_t r = b >= 0 ? sel[s0 + b] : -1;
    if (r >= 0)
      memcpy((uint8_t*)out + e * word, (const uint8_t*)column + r * word, word);
    else
      memset((uint8_t*)out + e * word, word == 8 ? 0xFF : 0, word);
    row[e] = (int32_t)r;
  }
}

// playout_pick_slot (the playout pick's own function) a lane an env, for the
// comparison with trials = 1, zero sums and leaf = the slot scores
void hc_playout_pick_slots(int64_t n, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld,
                           const int8_t* reward, int trials, const int32_t* sums, const float* leaf,
                           const uint8_t* black, int32_t* slot, float* score) {
  for (int64_t e = 0; e < n; ++e) {
    const int64_t s0 = e * k;
    slot[e] = playout_pick_slot(sel + s0, k, cap, value, ld, reward, sums + 4 * s0, leaf ? leaf + s0 * trials : nullptr,
                                trials, black[e] != 0, score + s0);
  }
}

}  // extern "C"
