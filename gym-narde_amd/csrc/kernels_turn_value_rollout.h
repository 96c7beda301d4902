// kernels_turn_value_rollout.h -- whole value-greedy FULL4 games in one launch, one net per colour
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_turn_lookahead.h and kernels_value_rollout.h: the level walk
// and its reducing consumer, the ply loop's carry, vr_net and vr_uniform are
// there); not a standalone header.
#pragma once

namespace {

// narde_turn_value_rollout: per env and ply what
// narde_turn_afterstates_scored, narde_turn_pick and narde_step_full do in
// five or six launches, in one loop of one wave.  A wave plays envs w,
// w + waves, ..., each for all its plies: the env's record stays in registers
// as a Side across the plies (every lane holds it: the rules run
// wave-uniformly), the statistics increments and the Philox block are carried
// in LDS (VrCarry).  A ply
//   takes its words and dice as k_step does (ply_draw_cached, dice_from);
//   takes the mover's net (vr_net; a colour with no net plays k_step's
//   random-legal turn, ply_full_words, from the same words);
//   makes the explore draw, once, before the walk;
//   walks the roll's levels on the record (turn_env, started from a position
//   as the lookahead's reply walks are) with kTurnFront nodes a level in LDS
//   and, if a level outgrows that, again with kTurnAftMax nodes a level in the
//   wave's own piece of the caller's slab -- both wave-uniform, exact for
//   every position;
//   hands the final level to turn_pick_level (below) in place of a store;
//   plays the row's play word (env_ply_full: the TimeLimit, the statistics,
//   the auto-reset) and stores the ply's outputs from lane 0.
// No row, feature or per-row value goes to memory.  The env-to-wave
// assignment is static: nothing spins and nothing is claimed with an atomic.
// The ply is tvr_ply below: k_turn_value_rollout_league (kernels_league.h)
// runs it through tvr_env_plies, k_turn_value_playout
// (kernels_turn_value_playout.h) in its own loop; k_turn_value_rollout, at the
// end of this file, still spells the same ply out (the reason is there).
static_assert(NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1) == (int64_t)kTurnSlabWave, "narde.h states the same slab piece");

struct TvrArgs {
  Planes pl;
  int n;
  Rng g;
  int max_steps;
  int plies;
  const float* __restrict__ eps;    // NULL: greedy
  const int64_t* __restrict__ tag;  // ply k's explore tag is *tag + k
  uint32_t k0, k1;                  // the explore draws' key
  uint8_t* __restrict__ dice;       // [plies][n][2]
  uint64_t* __restrict__ play;      // [plies][n]: the (4,2) int8 play, one word
  float* __restrict__ value;        // [plies][n]
  int32_t* __restrict__ reward;     // [plies][n]
  uint8_t* __restrict__ term;       // [plies][n]
  uint8_t* __restrict__ trunc;      // [plies][n]
  uint8_t* __restrict__ slab;       // [gridDim.x][kTurnSlabWave]
  uint4* __restrict__ records;      // [plies][n][2]: the record each ply found (the kRec kernels only)
};

// The row the mover plays, of the final level a walk of s under r left
// (nrows > 0 nodes of `level` sub-moves in pcur): the root forward of s, then
// 64 nodes at a time carried out, staged against it and scored, every value
// offered to the lane's best so far (RowBest's order is total: the butterfly
// over the lanes gives the row narde_turn_pick's serial scan gives) with the
// node's index in the level as its ordinal and its path as the payload; a
// terminal row is offered by its lane at its outcome.  The row count is known
// before the level is touched, so an explore ply stages and scores the one
// row of ordinal mulhi(r1, nrows).  All lanes of the wave call it with the
// same arguments; pk.b is the same in every lane.
__device__ __forceinline__ void turn_pick_level(const Side& s, const TurnRoot& r, const uint32_t* pcur, int nrows,
                                                int level, const ValNet& vn, ValStage& VS, TurnPick& pk, int lane) {
  const bool smallest = pk.smallest;
  RowBest b = row_best_none();
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  ValRoot vr;
  val_root(vr, vn, VS, ra, rb, lane);
  const int want = pk.explore ? (int)mulhi_u32(pk.r1, (uint32_t)nrows) : -1;  // wave-uniform
  const int g1 = want < 0 ? nrows : want + 1;
  for (int g0 = want < 0 ? 0 : want; g0 < g1; g0 += 64) {
    const int nr = min(64, g1 - g0);
    const bool act = lane < nr;
    const uint32_t path = act ? pcur[g0 + lane] : kTurnNoPath;
    Side c = s;
    turn_path_apply(c, path, act ? level : 0, r.dh, r.dl);
    int term, rew;
    step_end(c, false, term, rew);
    if (act) {
      uint4 ca, cb;
      side_to_record(c, ca, cb);
      val_stage_row(vn, VS, vr, lane, 0, 0, ca, cb, rew);  // (cap 0: nothing is stored)
      if (rew != 0) row_best_offer(b, val_outcome(rew, (cb.z >> 10) & 1u, 1), g0 + lane, path, smallest);
    }
    val_rows_each(vn, VS, vr, nr, [&](int q, float v) { row_best_offer(b, v, g0 + q, pcur[g0 + q], smallest); });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowBest p;
    p.x = __shfl_xor(b.x, o, 64);
    p.v = __shfl_xor(b.v, o, 64);
    p.ord = __shfl_xor(b.ord, o, 64);
    p.codes = (uint32_t)__shfl_xor((int)b.codes, o, 64);
    row_best_merge(b, p);
  }
  pk.b = b;
  pk.level = level;
  pk.dh = r.dh;
  pk.dl = r.dl;
}

// the walk of pk's position under its roll with `room` nodes a level and the
// pick of its final level; the row count, or -1 if a level outgrew room
__device__ __forceinline__ int turn_pick_roll(TurnPick& pk, uint64_t* knxt, uint32_t* pathA, uint32_t* pathB, int room,
                                              TurnScan& L, const ValNet& vn, ValStage& VS) {
  const TurnArgs none{};
  return turn_env<false, false, false, true, true>(none, 0, knxt, pathA, pathB, room, L, nullptr, &vn, &VS, nullptr,
                                                   &pk);
}

// wave `wave`'s piece of the caller's slab: a level's keys and its two path arrays
struct TurnSlab {
  uint64_t* key;
  uint32_t* pathA;
  uint32_t* pathB;
};
__device__ __forceinline__ TurnSlab turn_slab(uint8_t* slab, int wave) {
  uint64_t* const key = reinterpret_cast<uint64_t*>(slab + (size_t)wave * kTurnSlabWave);
  uint32_t* const pathA = reinterpret_cast<uint32_t*>(key + kTurnSlabKeys);
  return TurnSlab{key, pathA, pathA + kTurnAftMax};
}

// what a ply leaves for its caller besides the record it advanced
struct TvrPly {
  int d0, d1;
  bool black;     // the mover
  RowBest b;      // the row played (ord < 0: none)
  uint64_t play;  // the turn played: the row's play word, or the random-legal turn's
  TurnOut o;
  int term, trunc;
};

// Ply k of env index e's stream on s: the one FULL4 ply of the rollout, league
// and playout kernels (vr_ply's arguments, with the frontier in LDS and the
// wave's slab piece in place of the REF2 expansion's blocks).  All lanes of the
// wave call it with the same arguments.
template <bool kStats, class Nets>
__device__ __forceinline__ TvrPly tvr_ply(Side& s, const Rng& g, int e, int k, const Nets& nets, const VrExplore& ex,
                                          int max_steps, bool auto_reset, const TurnSlab& slab, TurnFrontLds& F,
                                          TurnScan& L, ValStage& VS, VrCarry& C, int lane) {
  TvrPly p;
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
  uint64_t pw = ~0ull;  // no row: the all -1 play
  if (has) {            // wave-uniform
    const ValNet vn = nets.net(p.black);
    uint32_t r1 = 0u;
    const bool explore = ex.on && explore_draw(ex.tag0 + (uint32_t)k, (uint32_t)e, ex.k0, ex.k1, ex.eps_q32, r1);
    // the values are white's: black plays the smallest
    TurnPick pk{{s, p.d0, p.d1, nullptr, p.black, 0.0f}, vr_uniform(explore ? 1u : 0u) != 0u, vr_uniform(r1),
                row_best_none(), 0, 0, 0};
    wave_lds_handoff();  // the last ply's reads of the frontier are done
    int nrows = turn_pick_roll(pk, F.key, F.path[0], F.path[1], kTurnFront, L, vn, VS);
    if (nrows < 0) {  // wave-uniform: the same walk in the wave's piece of the slab
      wave_lds_handoff();
      nrows = turn_pick_roll(pk, slab.key, slab.pathA, slab.pathB, kTurnAftMax, L, vn, VS);
    }
    // (kTurnAftMax bounds every level: nrows < 0 cannot happen twice; it would be a pass)
    if (nrows > 0) {
      p.b = pk.b;
      pw = turn_path_play_words(p.b.codes, pk.level, pk.dh, pk.dl);
    }
  }
  wave_lds_handoff();  // lane 0's block and increments, to every lane
  uint32_t R[4], r[4];
  vr_load4(C.R, R);
  ply_words_of(R, s.t, g.dice_mode, r);
  int4 st = make_int4(0, 0, 0, 0);
  if (kStats) st = C.st;
  if (has)  // wave-uniform
    env_ply_full(s, st, r, g.env0 + (uint32_t)e, g.k0, g.k1, false, 0, 0, g.dice_mode, true, pw, max_steps, auto_reset,
                 p.o, p.term, p.trunc);
  else  // narde_step_full(play = NULL)'s own turn (every lane the same env: its cooperative passes find 64 equal owners)
    ply_full_words(s, st, r, g.dice_mode, max_steps, auto_reset, p.o, p.term, p.trunc);
  p.play = has ? pw : p.o.played;
  wave_lds_handoff();  // (every lane has read the block and the increments)
  if (kStats && lane == 0) C.st = st;
  return p;
}

// env e's plies of a launch (vr_env_plies, whole turns); a wave plays several
// envs, one after the other
template <bool kRec, class Nets>
__device__ __forceinline__ void tvr_env_plies(const TvrArgs& a, int e, const Nets& nets, const TurnSlab& slab,
                                              TurnFrontLds& F, TurnScan& L, ValStage& VS, VrCarry& C, int lane) {
  Side s = side_from_record(a.pl.p0[e], a.pl.p1[e]);
  const VrExplore ex = vr_explore(a.eps, a.tag, a.k0, a.k1);
  wave_lds_handoff();  // (the last env's reads of the carry are done)
  if (lane == 0) C.st = make_int4(0, 0, 0, 0);
  for (int k = 0; k < a.plies; ++k) {
    const size_t ix = (size_t)k * (size_t)a.n + (size_t)e;
    if (kRec && lane == 0) vr_store_record(a.records, ix, s);
    const TvrPly p = tvr_ply<true>(s, a.g, e, k, nets, ex, a.max_steps, true, slab, F, L, VS, C, lane);
    if (lane == 0) {
      if (a.play) a.play[ix] = p.play;
      vr_store_ply(a, ix, p);
    }
  }
  if (lane == 0) vr_finish(a.pl, e, s, C);
}

// one-wave workgroups; wave w plays envs w, w + gridDim.x, ... (the LDS of
// k_turn_look<1> and the carry); kRec: a.records is written (vr_store_record).
// The one kernel that keeps its own text of tvr_env_plies and tvr_ply: over
// them it measured 0.2 to 1.0 % slower than this body, outside the runs' spread
// at B = 65,536 ("Tried"); the league and playout
// kernels did not.  A change to tvr_ply is made here too;
// tests/test_gpu_league.py holds the two equal byte for byte.
template <bool kRec>
__global__ void __launch_bounds__(64) k_turn_value_rollout(TvrArgs a, ValNet net_w, ValNet net_b, int has_w,
                                                           int has_b) {
  __shared__ TurnFrontLds F;
  __shared__ TurnScan L;
  __shared__ ValStage VS;
  __shared__ VrCarry C;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const int waves = (int)gridDim.x;
  uint8_t* const base = a.slab + (size_t)wave * kTurnSlabWave;
  uint64_t* const skey = reinterpret_cast<uint64_t*>(base);
  uint32_t* const spathA = reinterpret_cast<uint32_t*>(skey + kTurnSlabKeys);
  uint32_t* const spathB = spathA + kTurnAftMax;
  const uint64_t eps_q32 = a.eps ? eps_to_q32(*a.eps) : 0ull;
  const uint32_t tag0 = a.eps ? (uint32_t)*a.tag : 0u;
  for (int e = wave; e < a.n; e += waves) {
    Side s = side_from_record(a.pl.p0[e], a.pl.p1[e]);
    wave_lds_handoff();  // (the last env's reads of the carry are done)
    if (lane == 0) C.st = make_int4(0, 0, 0, 0);
    for (int k = 0; k < a.plies; ++k) {
      if (kRec && lane == 0) vr_store_record(a.records, (size_t)k * (size_t)a.n + (size_t)e, s);
      int d0, d1;
      {
        uint32_t R[4], r[4];
        if (k > 0) vr_load4(C.R, R);
        ply_draw_cached(a.g, s.t, (uint32_t)e, R, k == 0, r);
        if (lane == 0) C.R = make_uint4(R[0], R[1], R[2], R[3]);
        dice_from(r[0], a.g.dice_mode, d0, d1);
        d0 = (int)vr_uniform((uint32_t)d0);
        d1 = (int)vr_uniform((uint32_t)d1);
      }
      const bool black = vr_uniform(s.black) != 0u;
      const bool has = (black ? has_b : has_w) != 0;
      RowBest b = row_best_none();
      uint64_t pw = ~0ull;  // no row: the all -1 play
      if (has) {            // wave-uniform
        const ValNet vn = vr_net(black, net_w, net_b);
        uint32_t r1 = 0u;
        const bool explore = a.eps && explore_draw(tag0 + (uint32_t)k, (uint32_t)e, a.k0, a.k1, eps_q32, r1);
        // the values are white's: black plays the smallest
        TurnPick pk{{s, d0, d1, nullptr, black, 0.0f}, vr_uniform(explore ? 1u : 0u) != 0u, vr_uniform(r1),
                    row_best_none(), 0, 0, 0};
        wave_lds_handoff();  // the last ply's reads of the frontier are done
        int nrows = turn_pick_roll(pk, F.key, F.path[0], F.path[1], kTurnFront, L, vn, VS);
        if (nrows < 0) {  // wave-uniform: the same walk in the wave's piece of the slab
          wave_lds_handoff();
          nrows = turn_pick_roll(pk, skey, spathA, spathB, kTurnAftMax, L, vn, VS);
        }
        // (kTurnAftMax bounds every level: nrows < 0 cannot happen twice; it would be a pass)
        if (nrows > 0) {
          b = pk.b;
          pw = turn_path_play_words(b.codes, pk.level, pk.dh, pk.dl);
        }
      }
      wave_lds_handoff();  // lane 0's block and increments, to every lane
      uint32_t R[4], r[4];
      vr_load4(C.R, R);
      ply_words_of(R, s.t, a.g.dice_mode, r);
      const int4 st0 = C.st;
      int4 st = st0;
      TurnOut o;
      int term, trunc;
      if (has)  // wave-uniform
        env_ply_full(s, st, r, a.g.env0 + (uint32_t)e, a.g.k0, a.g.k1, false, 0, 0, a.g.dice_mode, true, pw, a.max_steps,
                     true, o, term, trunc);
      else  // narde_step_full(play = NULL)'s own turn (every lane the same env: its cooperative passes find 64 equal owners)
        ply_full_words(s, st, r, a.g.dice_mode, a.max_steps, true, o, term, trunc);
      wave_lds_handoff();  // (every lane has read the increments)
      if (lane == 0) {
        C.st = st;
        const size_t ix = (size_t)k * (size_t)a.n + (size_t)e;
        if (a.dice) {
          a.dice[2 * ix] = (uint8_t)d0;
          a.dice[2 * ix + 1] = (uint8_t)d1;
        }
        if (a.play) a.play[ix] = has ? pw : o.played;
        if (a.value) a.value[ix] = b.ord >= 0 ? b.v : __builtin_nanf("");
        if (a.reward) a.reward[ix] = o.reward;
        if (a.term) a.term[ix] = (uint8_t)term;
        if (a.trunc) a.trunc[ix] = (uint8_t)trunc;
      }
    }
    if (lane == 0) {
      uint4 ra, rb;
      side_to_record(s, ra, rb);
      a.pl.p0[e] = ra;
      a.pl.p1[e] = rb;
      add_stats(a.pl.stats, e, C.st);  // (lane 0's own last write)
    }
  }
}

}  // namespace
