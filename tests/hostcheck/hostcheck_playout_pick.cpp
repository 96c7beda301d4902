// hostcheck_playout_pick.cpp -- TEST-ONLY host build of playout-greedy play
// (gym-narde_amd/csrc/kernels_playout_pick.h), both
// rule sets.
//
// Runs serially the functions the records fills, k_rows_topk and
// k_playout_pick run on the device: an env's rows (REF2: kept_plays,
// play_afterstate; FULL4: the level walk, turn_path_apply, step_end), each
// row's narrow outputs, its value against the env's record as root (root_of,
// value_of: the scored fill's arithmetic) and its record in the public form
// (side_to_record, record_close_step); the top-K rounds with the rows offered
// in the lanes the device holds them in and merged by the same butterfly
// (topk_offers, argmax_takes); the pick over the playouts' sums
// (playout_pick_slot, the device's own function).  The rows, roots and values
// are hostcheck_lookahead.cpp's and hostcheck_turn_afterstates.cpp's own
// functions, compiled in through hostcheck_value_playout.cpp, whose
// hc_value_playout this library exports as well.
// tests/test_playout_pick_cpu.py compares the results with restatements over
// the C oracle and numpy.  Never loaded by the product.
#include "hostcheck_value_playout.cpp"

extern "C" {

uint32_t hc_record_none_word6() { return kRecordNoneWord6; }

// narde_afterstates_records (full 0) / narde_turn_afterstates_records (full 1)
// on the host: n envs (board, off, ft, player, elapsed; the ply counter t),
// dice in roll order, net NULL for the records alone.  Rows in CSR order,
// those below cap written: row_env i32, action (codes i16[2] or play i8[4][2]),
// reward i8, value f32 (with a net), records u32[8].  Returns offsets[n].
int64_t hc_records(int full, int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft,
                   const int8_t* player, const uint16_t* elapsed, uint32_t t, const uint8_t* dice, int64_t cap,
                   const NetIn* in, int32_t* offsets, int32_t* row_env, void* action, int8_t* reward, float* value,
                   uint32_t* records) {
  Net net{};
  if (in) net = Net{in->w1t, in->b1, in->w2, in->b2, in->ld, in->hidden, in->hidden_act, in->out_act};
  int64_t row = 0;
  offsets[0] = 0;
  std::vector<Node> rows;
  for (int64_t i = 0; i < n; ++i) {
    uint4 ea, eb;
    record_from_board(board + i * 24, off[2 * i], off[2 * i + 1], ft[2 * i], ft[2 * i + 1], player[i], elapsed[i], t, ea,
                      eb);
    const Side s = side_from_record(ea, eb);
    const int d0 = dice[2 * i], d1 = dice[2 * i + 1];
    Root root;
    bool rooted = false;
    // a kept row: the afterstate c, its reward
    auto emit = [&](const Side& c, int rew, auto&& store_action) {
      const int64_t R = row++;
      if (R >= cap) return;
      row_env[R] = (int32_t)i;
      store_action(R);
      reward[R] = (int8_t)rew;
      uint4 ra, rb;
      side_to_record(c, ra, rb);
      if (in) {
        if (!rooted) {
          root_of(net, ea, eb, root);
          rooted = true;
        }
        value[R] = rew != 0 ? val_outcome(rew, (rb.z >> 10) & 1u, 1) : value_of(net, root, ra, rb);
      }
      record_close_step(rb);
      memcpy(records + 8 * R, &ra, 16);
      memcpy(records + 8 * R + 4, &rb, 16);
    };
    if (full) {
      rows.clear();
      int M = 0, fr;
      if (d0 >= 1 && d0 <= 6 && d1 >= 1 && d1 <= 6) M = turn_levels(s, d0, d1, rows, fr);
      const int dh = d0 > d1 ? d0 : d1, dl = d0 > d1 ? d1 : d0;
      for (const Node& nd : rows) {
        Side c = s;
        turn_path_apply(c, nd.path, M, dh, dl);
        int term, rew;
        step_end(c, false, term, rew);
        emit(c, rew, [&](int64_t R) {
          const uint64_t pw = turn_path_play(nd.path, M, dh, dl);
          memcpy((int8_t*)action + R * 8, &pw, 8);
        });
      }
    } else {
      kept_plays(s, d0, d1, [&](const Play& y) {
        Side c = s;
        int term, rew, c1, c2;
        play_afterstate(c, y, term, rew);
        play_codes(y, c1, c2);
        emit(c, rew, [&](int64_t R) {
          ((int16_t*)action)[2 * R] = (int16_t)c1;
          ((int16_t*)action)[2 * R + 1] = (int16_t)c2;
        });
      });
    }
    offsets[i + 1] = (int32_t)row;
  }
  return row;
}

// narde_rows_topk on the host, a wave an env: black u8[n] = the env's mover
// is black.  sel i32[n][k]; roots u32[n][k][8] with records, else NULL.
void hc_rows_topk(int64_t n, const int32_t* offsets, int64_t cap, const float* value, int64_t ld,
                  const uint8_t* black, int perspective, int k, const uint32_t* records, int32_t* sel,
                  uint32_t* roots) {
  for (int64_t e = 0; e < n; ++e) {
    const int64_t r0 = offsets[e];
    const int64_t r1 = offsets[e + 1] < cap ? offsets[e + 1] : cap;
    const int cnt = r1 > r0 ? (int)(r1 - r0) : 0;
    const bool smallest = perspective == 1 && black[e];
    float px = 0.0f;
    int pi = -1;
    for (int i = 0; i < k; ++i) {
      float bx[64];
      int bi[64];
      for (int lane = 0; lane < 64; ++lane) {
        bx[lane] = 0.0f;
        bi[lane] = -1;
        if (i < cnt)
          for (int q = lane; q < cnt; q += 64) {
            const float v = value[(r0 + q) * ld];
            const float x = smallest ? -v : v;
            if (topk_offers(px, pi, x, q) && argmax_takes(x, q, bx[lane], bi[lane])) {
              bx[lane] = x;
              bi[lane] = q;
            }
          }
      }
      if (i < cnt)
        for (int o = 32; o > 0; o >>= 1) {
          float nx[64];
          int ni[64];
          for (int lane = 0; lane < 64; ++lane) {
            nx[lane] = bx[lane];
            ni[lane] = bi[lane];
            if (argmax_takes(bx[lane ^ o], bi[lane ^ o], bx[lane], bi[lane])) {
              nx[lane] = bx[lane ^ o];
              ni[lane] = bi[lane ^ o];
            }
          }
          memcpy(bx, nx, sizeof bx);
          memcpy(bi, ni, sizeof bi);
        }
      px = bx[0];
      pi = bi[0];
      const int64_t row = bi[0] >= 0 ? r0 + bi[0] : -1;
      const int64_t slot = e * k + i;
      sel[slot] = (int32_t)row;
      if (roots) {
        if (row >= 0) {
          memcpy(roots + 8 * slot, records + 8 * row, 32);
        } else {
          memset(roots + 8 * slot, 0, 32);
          roots[8 * slot + 6] = kRecordNoneWord6;
        }
      }
    }
  }
}

// the picks' own loop (kernels_rows.h aft_pick_row, epsilon NULL): row i32[n]
void hc_pick_rows(int64_t n, const int32_t* offsets, int64_t cap, const float* value, int64_t ld,
                  const uint8_t* black, int perspective, int32_t* row) {
  for (int64_t e = 0; e < n; ++e) {
    const int64_t r0 = offsets[e];
    const int64_t r1 = offsets[e + 1] < cap ? offsets[e + 1] : cap;
    const int cnt = r1 > r0 ? (int)(r1 - r0) : 0;
    const bool smallest = perspective == 1 && black[e];
    float best = 0.0f;
    int bi = -1;
    for (int q = 0; q < cnt; ++q) {
      const float v = value[(r0 + q) * ld];
      const float x = smallest ? -v : v;
      if (argmax_takes(x, q, best, bi)) {
        best = x;
        bi = q;
      }
    }
    row[e] = cnt > 0 ? (int32_t)(r0 + bi) : -1;
  }
}

// narde_playout_pick / narde_turn_playout_pick on the host: words of `word`
// bytes (4: the two codes, no row 0; 8: the play, no row -1) from column to out
void hc_playout_pick(int64_t n, int k, const int32_t* sel, int64_t cap, const float* value, int64_t ld,
                     const int8_t* reward, const void* column, int word, int trials, const int32_t* sums,
                     const float* leaf, const uint8_t* black, void* out, int32_t* row, float* score) {
  for (int64_t e = 0; e < n; ++e) {
    const int64_t s0 = e * k;
    const int b = playout_pick_slot(sel + s0, k, cap, value, ld, reward, sums + 4 * s0,
                                    leaf ? leaf + s0 * trials : nullptr, trials, black[e] != 0, score + s0);
    const int64_t r = b >= 0 ? sel[s0 + b] : -1;
    if (r >= 0)
      memcpy((uint8_t*)out + e * word, (const uint8_t*)column + r * word, word);
    else
      memset((uint8_t*)out + e * word, word == 8 ? 0xFF : 0, word);
    row[e] = (int32_t)r;
  }
}

// board_from_record on n records: board i8[24], off u8[2], ft u8[2], player i8,
// elapsed u16, t u32
void hc_decode_records(int64_t n, const uint32_t* records, int8_t* board, uint8_t* off, uint8_t* ft, int8_t* player,
                       uint16_t* elapsed, uint32_t* t) {
  for (int64_t i = 0; i < n; ++i) {
    uint4 a, b;
    memcpy(&a, records + 8 * i, 16);
    memcpy(&b, records + 8 * i + 4, 16);
    board_from_record(a, b, board + 24 * i, off + 2 * i, ft + 2 * i, player + i, elapsed + i);
    t[i] = b.w;
  }
}

}  // extern "C"
