// kernels_value_rollout.h -- whole value-greedy games in one launch, one net per colour
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_lookahead.h: the play enumeration and the scored rows'
// helpers are k_aft_look's); not a standalone header.
#pragma once

namespace {

// narde_value_rollout: per env and ply what narde_afterstates_scored,
// narde_afterstate_pick and narde_step do in four or five launches, in one
// loop of one wave.  The env's record stays in registers as a Side across
// the plies (every lane holds it: the rules run wave-uniformly); the
// statistics increments and the Philox block are carried in LDS (VrCarry).
// A ply
//   takes its words and dice as k_step does (ply_draw_cached, dice_from);
//   takes the mover's net (a scalar select on s.black; a colour with no net
//   plays the random-legal policy inside env_ply, from the same words);
//   expands the roll on the record as k_aft_look expands a row's replies
//   (val_root, aft_entries, aft_chunks, val_stage_row, val_rows_each) and
//   keeps, in place of a store, each lane's best row so far (narde_rules.h
//   RowBest: aft_pick_row's order, which is total, so the butterfly over the
//   lanes gives the row aft_pick_row's serial scan gives);
//   plays the row's codes (env_ply: the TimeLimit, the statistics, the
//   auto-reset) and stores the ply's outputs from lane 0.
// The explore draw is aft_pick_row's, once an env and ply; the uniform row
// needs the row count first, so a ply whose draw fires counts its rows in a
// first pass of aft_chunks (no row is scored) and scores the one row of
// ordinal mulhi(r1, count) in a second: greedy plies pay nothing for it.
// No row, feature or per-row value goes to memory.  An env is one wave
// whatever B: splitting an env's chunks over several waves for tiny B is not
// done (section 19.5).
// The ply is vr_ply below, the one REF2 ply: k_value_rollout and
// k_value_rollout_league (kernels_league.h) run it through vr_env_plies,
// k_value_playout (kernels_value_playout.h) in its own loop.  vr_store_ply and
// vr_finish are the FULL4 loop's too.
struct VrArgs {
  Planes pl;
  int n;
  Rng g;
  int max_steps;
  int plies;
  const float* __restrict__ eps;    // NULL: greedy
  const int64_t* __restrict__ tag;  // ply k's explore tag is *tag + k
  uint32_t k0, k1;                  // the explore draws' key
  uint8_t* __restrict__ dice;       // [plies][n][2]
  int16_t* __restrict__ actions;    // [plies][n][2]
  float* __restrict__ value;        // [plies][n]
  int32_t* __restrict__ reward;     // [plies][n]
  uint8_t* __restrict__ term;       // [plies][n]
  uint8_t* __restrict__ trunc;      // [plies][n]
  uint4* __restrict__ records;      // [plies][n][2]: the record each ply found (the kRec kernels only)
};

struct alignas(16) VrStage {  // per wave: a chunk's kept rows' codes, by rank
  uint32_t codes[64];
};

// What the plies' loop carries besides the record and no ply's expansion
// needs -- the ply stream's Philox block (it serves two plies) and the
// statistics increments --, kept in LDS so that the expansion has the
// registers k_aft_look has: lane 0 writes, every lane reads.
struct alignas(16) VrCarry {
  uint4 R;
  int4 st;
};
__device__ __forceinline__ void vr_load4(const uint4& v, uint32_t w[4]) {
  const uint4 x = v;
  w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
}

// a value every lane holds alike, as a scalar
__device__ __forceinline__ uint32_t vr_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// the mover's net: a scalar select a field (black is wave-uniform), not two
// copies of the expansion
__device__ __forceinline__ ValNet vr_net(bool black, const ValNet& w, const ValNet& b) {
  return ValNet{black ? b.w1t : w.w1t,
                black ? b.ld : w.ld,
                black ? b.b1 : w.b1,
                black ? b.w2 : w.w2,
                black ? b.b2 : w.b2,
                black ? b.hidden : w.hidden,
                black ? b.hidden_act : w.hidden_act,
                black ? b.out_act : w.out_act,
                1,
                nullptr};
}

// the row the mover of s plays on the roll (d0, d1) under vn: b.ord < 0 if
// the roll has no row.  want_explore: the uniform row of ordinal
// mulhi(r1, count) instead of the best.  All lanes of the wave call it with
// the same arguments; the result is the same in every lane.
__device__ __forceinline__ RowBest vr_choose(const Side& s, int d0, int d1, const ValNet& vn, AftScan& L, ValStage& VS,
                                             VrStage& CS, int lane, bool want_explore, uint32_t r1) {
  RowBest b = row_best_none();
  Legal l;
  legal2(s, d0, d1, l);
  const int total = aft_entries(s, d0, d1, l, L, lane);
  if (total == 0) return b;  // wave-uniform: no play
  int want = -1;
  if (want_explore) {  // wave-uniform
    const int cnt = aft_chunks(l, total, L, lane, [](int, bool, int, int, const Play&) {});
    if (cnt == 0) return b;
    want = (int)mulhi_u32(r1, (uint32_t)cnt);
  }
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  ValRoot vr;
  val_root(vr, vn, VS, ra, rb, lane);
  const bool smallest = s.black != 0u;  // the values are white's: black plays the smallest
  aft_chunks(l, total, L, lane, [&](int nkept, bool keep, int rank, int nnew, const Play& y) {
    // greedy: every kept row of the chunk, staged by rank; explore: the one
    // row of ordinal `want`, staged first, in the chunk that holds it
    if (want >= 0 && (want < nkept || want >= nkept + nnew)) return;  // wave-uniform
    const bool sel = want < 0 ? keep : (keep && nkept + rank == want);
    const int slot = want < 0 ? rank : 0;
    const int ord0 = want < 0 ? nkept : want;
    if (sel) {
      Side c = s;
      int term, rew, c1, c2;
      play_afterstate(c, y, term, rew);
      play_codes(y, c1, c2);
      uint4 ca, cb;
      side_to_record(c, ca, cb);
      val_stage_row(vn, VS, vr, slot, 0, 0, ca, cb, rew);  // (cap 0: nothing is stored)
      const uint32_t pk = pack_codes(c1, c2);
      CS.codes[slot] = pk;
      if (rew != 0) row_best_offer(b, val_outcome(rew, (cb.z >> 10) & 1u, 1), ord0 + slot, pk, smallest);
    }
    val_rows_each(vn, VS, vr, want < 0 ? nnew : 1,
                  [&](int q, float v) { row_best_offer(b, v, ord0 + q, CS.codes[q], smallest); });
  });
  // the lanes' bests -> the wave's, in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowBest p;
    p.x = __shfl_xor(b.x, o, 64);
    p.v = __shfl_xor(b.v, o, 64);
    p.ord = __shfl_xor(b.ord, o, 64);
    p.codes = (uint32_t)__shfl_xor((int)b.codes, o, 64);
    row_best_merge(b, p);
  }
  return b;
}

// ply k's record of env e as the ply found it, from lane 0 (the windowed TD
// update's input): stored before the roll is applied,
// so nothing of it is held across the expansion
__device__ __forceinline__ void vr_store_record(uint4* __restrict__ records, size_t ix, const Side& s) {
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  records[2 * ix] = ra;
  records[2 * ix + 1] = rb;
}

// the explore draws' parameters of a launch (on = false: every ply is greedy)
struct VrExplore {
  bool on;
  uint64_t eps_q32;
  uint32_t tag0, k0, k1;  // ply k's tag is tag0 + k; the draws' key
};
__device__ __forceinline__ VrExplore vr_explore(const float* eps, const int64_t* tag, uint32_t k0, uint32_t k1) {
  return VrExplore{eps != nullptr, eps ? eps_to_q32(*eps) : 0ull, eps ? (uint32_t)*tag : 0u, k0, k1};
}

// Where the mover's net comes from: has(black) says whether that colour has a
// net (wave-uniform; none: the random-legal policy), net(black) gives it with
// every field a scalar.  The launch's two nets here; the league's table entry
// of the env's pair in kernels_league.h (LeagueNets).
struct VrTwoNets {
  const ValNet& w;
  const ValNet& b;
  int has_w, has_b;
  __device__ __forceinline__ bool has(bool black) const { return (black ? has_b : has_w) != 0; }
  __device__ __forceinline__ ValNet net(bool black) const { return vr_net(black, w, b); }
};

// what a ply leaves for its caller besides the record it advanced
struct VrPly {
  int d0, d1;
  bool black;  // the mover
  RowBest b;   // the row played (ord < 0: none)
  StepOut o;
  int term, trunc;
};

// Ply k of env index e's stream on s: the one REF2 ply of the rollout, league
// and playout kernels.  kStats: the statistics increments are carried in C.st
// across the plies (the caller zeroes it before ply 0); otherwise they are
// dropped.  All lanes of the wave call it with the same arguments.
template <bool kStats, class Nets>
__device__ __forceinline__ VrPly vr_ply(Side& s, const Rng& g, int e, int k, const Nets& nets, const VrExplore& ex,
                                        int max_steps, bool auto_reset, AftScan& L, ValStage& VS, VrStage& CS,
                                        VrCarry& C, int lane) {
  VrPly p;
  {
    uint32_t R[4], r[4];
    if (k > 0) vr_load4(C.R, R);
    ply_draw_cached(g, s.t, (uint32_t)e, R, k == 0, r);
    if (lane == 0) C.R = make_uint4(R[0], R[1], R[2], R[3]);
    dice_from(r[0], g.dice_mode, p.d0, p.d1);
    p.d0 = (int)vr_uniform((uint32_t)p.d0);
    p.d1 = (int)vr_uniform((uint32_t)p.d1);
  }
  p.black = vr_uniform(s.black) != 0u;
  const bool has = nets.has(p.black);
  p.b = row_best_none();
  if (has) {  // wave-uniform
    const ValNet vn = nets.net(p.black);
    uint32_t r1 = 0u;
    const bool explore = ex.on && explore_draw(ex.tag0 + (uint32_t)k, (uint32_t)e, ex.k0, ex.k1, ex.eps_q32, r1);
    p.b = vr_choose(s, p.d0, p.d1, vn, L, VS, CS, lane, vr_uniform(explore ? 1u : 0u) != 0u, vr_uniform(r1));
  }
  const int c1 = (int)(int16_t)(p.b.codes & 0xFFFFu), c2 = (int)(int16_t)(p.b.codes >> 16);  // (no row: 0, 0)
  wave_lds_handoff();  // lane 0's block and increments, to every lane
  uint32_t R[4], r[4];
  vr_load4(C.R, R);
  ply_words_of(R, s.t, g.dice_mode, r);
  int4 st = make_int4(0, 0, 0, 0);
  if (kStats) st = C.st;
  env_ply(s, st, r, false, 0, 0, g.dice_mode, !has, c1, c2, max_steps, auto_reset, p.o, p.term, p.trunc);
  wave_lds_handoff();  // (every lane has read the block and the increments)
  if (kStats && lane == 0) C.st = st;
  return p;
}

// ply k's outputs of env e that both rule sets have, from lane 0 (the action
// or play column is the caller's): Args is VrArgs or TvrArgs, Ply VrPly or TvrPly
template <class Args, class Ply>
__device__ __forceinline__ void vr_store_ply(const Args& a, size_t ix, const Ply& p) {
  if (a.dice) {
    a.dice[2 * ix] = (uint8_t)p.d0;
    a.dice[2 * ix + 1] = (uint8_t)p.d1;
  }
  if (a.value) a.value[ix] = p.b.ord >= 0 ? p.b.v : __builtin_nanf("");
  if (a.reward) a.reward[ix] = p.o.reward;
  if (a.term) a.term[ix] = (uint8_t)p.term;
  if (a.trunc) a.trunc[ix] = (uint8_t)p.trunc;
}

// the end of env e's plies, from lane 0: the record back to the planes and the
// carried increments (lane 0's own last write) to the statistics
__device__ __forceinline__ void vr_finish(const Planes& pl, int e, const Side& s, const VrCarry& C) {
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  pl.p0[e] = ra;
  pl.p1[e] = rb;
  add_stats(pl.stats, e, C.st);
}

// env e's plies of a launch: the record stays in registers across them; kRec:
// a.records is written (the no-records instantiations hold no trace of it)
template <bool kRec, class Nets>
__device__ __forceinline__ void vr_env_plies(const VrArgs& a, int e, const Nets& nets, AftScan& L, ValStage& VS,
                                             VrStage& CS, VrCarry& C, int lane) {
  Side s = side_from_record(a.pl.p0[e], a.pl.p1[e]);
  const VrExplore ex = vr_explore(a.eps, a.tag, a.k0, a.k1);
  if (lane == 0) C.st = make_int4(0, 0, 0, 0);
  for (int k = 0; k < a.plies; ++k) {
    const size_t ix = (size_t)k * (size_t)a.n + (size_t)e;
    if (kRec && lane == 0) vr_store_record(a.records, ix, s);
    const VrPly p = vr_ply<true>(s, a.g, e, k, nets, ex, a.max_steps, true, L, VS, CS, C, lane);
    if (lane == 0) {
      if (a.actions) reinterpret_cast<uint32_t*>(a.actions)[ix] = pack_codes(p.o.code1, p.o.code2);
      vr_store_ply(a, ix, p);
    }
  }
  if (lane == 0) vr_finish(a.pl, e, s, C);
}

// one wave per env, an env per workgroup (k_aft_look<1>'s LDS and the codes)
template <bool kRec>
__global__ void __launch_bounds__(64) k_value_rollout(VrArgs a, ValNet net_w, ValNet net_b, int has_w, int has_b) {
  __shared__ AftScan L;
  __shared__ ValStage VS;
  __shared__ VrStage CS;
  __shared__ VrCarry C;
  const int e = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  if (e >= a.n) return;
  vr_env_plies<kRec>(a, e, VrTwoNets{net_w, net_b, has_w, has_b}, L, VS, CS, C, threadIdx.x & 63);
}

}  // namespace
