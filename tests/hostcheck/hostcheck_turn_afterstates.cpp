// hostcheck_turn_afterstates.cpp -- TEST-ONLY host build of the FULL4 turn
// afterstate rules layer (gym-narde_amd/csrc/narde_rules.h "FULL4 turn
// afterstates").
//
// Walks each env's levels serially through the functions the kernels
// (kernels_turn_afterstates.h) run a lane per node: turn_root,
// turn_path_apply, turn_node_lists, turn_child, turn_path_key's dedupe,
// turn_path_play, step_end, and the 198-float row by tes_value.
// tests/test_turn_afterstates_cpu.py compares the ordered rows with an
// enumerator over the C oracle.  Never loaded by the product.
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "../../gym-narde_amd/csrc/narde_rules.h"
#include "hostcheck_rows.h"

using namespace narde;

namespace {

struct Node {
  uint32_t path;
  uint64_t key;
};

// the rows' nodes (level M, less the lower die's at M = 1 when the higher
// has one); returns M.  front: the largest level met.
int turn_levels(const Side& s, int d0, int d1, std::vector<Node>& rows, int& front) {
  const TurnRoot r = turn_root(s, d0, d1);
  std::vector<Node> cur{{kTurnNoPath, 0ull}}, nxt;
  int level = 0, nh1 = 0;
  front = 0;
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
        if (!seen) nxt.push_back({cp, key});
      }
    }
    if (nxt.empty()) break;
    cur.swap(nxt);
    front = (int)cur.size() > front ? (int)cur.size() : front;
  }
  rows.clear();
  if (level == 0) return 0;
  rows = cur;
  if (r.dh != r.dl && level == 1 && nh1 > 0) rows.resize(nh1);
  return level;
}

}  // namespace

extern "C" {

int hc_turn_aft_max() { return kTurnAftMax; }

// Rows in CSR order: env i's rows are offsets[i] .. offsets[i + 1] - 1 (true
// counts); rows below cap are written: play i8[4][2], board i8[24]
// (absolute), off u8[2], player i8 (after the turn), reward i8, feat
// f32[198].  front[i] = the env's largest level.  Returns offsets[n].
int64_t hc_turn_afterstates(int64_t n, const int8_t* board, const uint8_t* off, const uint8_t* ft,
                            const int8_t* player, const uint8_t* dice, int64_t cap, int32_t* offsets, int32_t* front,
                            int8_t* play, int8_t* boards, uint8_t* offs, int8_t* players, int8_t* reward,
                            float* feat) {
  int64_t row = 0;
  offsets[0] = 0;
  std::vector<Node> rows;
  for (int64_t i = 0; i < n; ++i) {
    const int d0 = dice[2 * i], d1 = dice[2 * i + 1];
    front[i] = 0;
    if (d0 >= 1 && d0 <= 6 && d1 >= 1 && d1 <= 6) {
      const Side s = load_side(board + i * 24, off + 2 * i, ft + 2 * i, player[i]);
      const int dh = d0 > d1 ? d0 : d1, dl = d0 > d1 ? d1 : d0;
      int fr;
      const int M = turn_levels(s, d0, d1, rows, fr);
      front[i] = fr;
      for (const Node& nd : rows) {
        if (row < cap) {
          Side c = s;
          turn_path_apply(c, nd.path, M, dh, dl);
          int term, rew;
          step_end(c, false, term, rew);
          const uint64_t pw = turn_path_play(nd.path, M, dh, dl);
          memcpy(play + row * 8, &pw, 8);
          write_row(c, rew, row, boards, offs, players, reward, feat);
        }
        ++row;
      }
    }
    offsets[i + 1] = (int32_t)row;
  }
  return row;
}

// turn_path_key against the records on every sub-move sequence of one
// state, level by level (every path of the raw lists, no dedupe): within a
// level two paths must share a key iff they leave the same record (and, at
// level 1 of two different dice, the same die).  Checked through both maps
// key -> record and record -> key, which is the all-pairs statement.
// Returns the number of paths that break it; *paths = the paths checked.
int64_t hc_turn_key_pairs(const int8_t* board, const uint8_t* off, const uint8_t* ft, int8_t player,
                          const uint8_t* dice, int64_t* paths) {
  const Side s = load_side(board, off, ft, player);
  const TurnRoot r = turn_root(s, dice[0], dice[1]);
  using Rec = std::array<uint32_t, 9>;
  std::vector<uint32_t> cur{kTurnNoPath}, nxt;
  int64_t bad = 0;
  *paths = 0;
  for (int level = 0; level < r.depth && !cur.empty(); ++level) {
    nxt.clear();
    std::map<uint64_t, Rec> by_key;
    std::map<Rec, uint64_t> by_rec;
    for (const uint32_t path : cur) {
      Side c = s;
      turn_path_apply(c, path, level, r.dh, r.dl);
      uint32_t w0, w1;
      turn_node_lists(c, path, level, r, w0, w1);
      const int cnt = __builtin_popcount(w0 & MASK24) + __builtin_popcount(w1 & MASK24);
      for (int j = 0; j < cnt; ++j) {
        const uint32_t cp = turn_child(path, level, w0, w1, j);
        const bool die_left = r.dh != r.dl && level == 0;
        const uint64_t key = turn_path_key(cp, level + 1, r.dh, r.dl, die_left);
        Side k = s;
        turn_path_apply(k, cp, level + 1, r.dh, r.dl);
        uint4 ra, rb;
        side_to_record(k, ra, rb);
        const Rec rec{ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w, die_left ? ((cp >> 7) & 1u) : 0u};
        const auto a = by_key.emplace(key, rec);
        const auto b = by_rec.emplace(rec, key);
        bad += (a.first->second != rec || b.first->second != key) ? 1 : 0;
        nxt.push_back(cp);
        ++*paths;
      }
    }
    cur.swap(nxt);
  }
  return bad;
}

}  // extern "C"
