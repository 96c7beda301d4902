// kernels_league.h -- round-robin leagues in one launch: a value net per env and colour
// Part of the one translation unit narde.hip (included there, in order, last:
// the two value rollouts' plies -- vr_choose, turn_pick_roll, the carry, the
// record store -- are kernels_value_rollout.h's and
// kernels_turn_value_rollout.h's); not a standalone header.
#pragma once

namespace {

// A table entry: the kernels' view of one net (ValNet without the two fields
// the rollouts fix: perspective 1, no value pointer), padded to the 64 B
// narde.h states.  The weights stay where they are: the entry holds pointers.
struct alignas(16) LeagueNet {
  const float* w1t;  // [198][ld]
  int64_t ld;
  const float* b1;  // [hidden]
  const float* w2;  // [hidden]
  const float* b2;  // [1]
  int hidden, hidden_act, out_act, pad;
};
static_assert(sizeof(LeagueNet) == NARDE_LEAGUE_TABLE_BYTES(1), "narde.h states the same entry");

// narde_net_table's launch: kLeagueBatch entries travel by value in the
// kernel's arguments (1 KiB: the 64 nets of a full table do not fit one
// launch's argument block), one thread an entry
constexpr int kLeagueBatch = 16;
struct LeagueBatch {
  LeagueNet n[kLeagueBatch];
};

__global__ void __launch_bounds__(64) k_net_table_write(LeagueBatch b, int count, LeagueNet* __restrict__ table) {
  const int i = (int)threadIdx.x;
  if (i >= count) return;
  // (static indices: the argument block is not copied to scratch to be indexed)
#pragma unroll
  for (int j = 0; j < kLeagueBatch; ++j)
    if (i == j) table[j] = b.n[j];
}

// a weight pointer out of an entry: device global memory, said so -- a pointer
// loaded from memory is generic to the compiler, and the scoring's loads
// through it would be flat loads where the two-net kernels' are global loads
__device__ __forceinline__ const float* league_global(const float* p) {
  return (const float*)(const __attribute__((address_space(1))) float*)reinterpret_cast<uintptr_t>(p);
}

// the mover's net: entry idx of the table (idx is wave-uniform and inside the
// table: the caller has tested it), read through the constant address space --
// the table is not written while the kernel runs --, so a scalar load, and
// every field a scalar as vr_net's select keeps them
__device__ __forceinline__ ValNet league_net(const LeagueNet* __restrict__ table, int idx) {
  typedef const __attribute__((address_space(4))) LeagueNet* Entry;
  const Entry t = (Entry)reinterpret_cast<uintptr_t>(table) + idx;
  return ValNet{league_global(t->w1t),
                t->ld,
                league_global(t->b1),
                league_global(t->w2),
                league_global(t->b2),
                t->hidden,
                t->hidden_act,
                t->out_act,
                1,
                nullptr};
}

// what the league kernels take besides the rollouts' own arguments: env e's
// white plies are net white[e]'s, its black plies net black[e]'s; an index
// outside 0 .. n_nets - 1 is the random-legal policy (no entry is read)
struct LeagueArgs {
  const LeagueNet* __restrict__ table;
  int n_nets;
  const int32_t* __restrict__ white;  // [n]
  const int32_t* __restrict__ black;  // [n]
};

// k_value_rollout's ply loop with the mover's net taken from the table: the
// env's pair is read once, the mover's entry once a ply (wave-uniformly)
template <bool kRec>
__global__ void __launch_bounds__(64) k_value_rollout_league(VrArgs a, LeagueArgs lg) {
  __shared__ AftScan L;
  __shared__ ValStage VS;
  __shared__ VrStage CS;
  __shared__ VrCarry C;
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  if (e >= a.n) return;
  Side s = side_from_record(a.pl.p0[e], a.pl.p1[e]);
  const int iw = (int)vr_uniform((uint32_t)lg.white[e]), ib = (int)vr_uniform((uint32_t)lg.black[e]);
  const uint64_t eps_q32 = a.eps ? eps_to_q32(*a.eps) : 0ull;
  const uint32_t tag0 = a.eps ? (uint32_t)*a.tag : 0u;
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
    const int idx = black ? ib : iw;
    const bool has = (uint32_t)idx < (uint32_t)lg.n_nets;
    RowBest b = row_best_none();
    if (has) {  // wave-uniform
      const ValNet vn = league_net(lg.table, idx);
      uint32_t r1 = 0u;
      const bool explore = a.eps && explore_draw(tag0 + (uint32_t)k, (uint32_t)e, a.k0, a.k1, eps_q32, r1);
      b = vr_choose(s, d0, d1, vn, L, VS, CS, lane, vr_uniform(explore ? 1u : 0u) != 0u, vr_uniform(r1));
    }
    const int c1 = (int)(int16_t)(b.codes & 0xFFFFu), c2 = (int)(int16_t)(b.codes >> 16);  // (no row: 0, 0)
    wave_lds_handoff();  // lane 0's block and increments, to every lane
    uint32_t R[4], r[4];
    vr_load4(C.R, R);
    ply_words_of(R, s.t, a.g.dice_mode, r);
    const int4 st0 = C.st;
    int4 st = st0;
    StepOut o;
    int term, trunc;
    env_ply(s, st, r, false, 0, 0, a.g.dice_mode, !has, c1, c2, a.max_steps, true, o, term, trunc);
    wave_lds_handoff();  // (every lane has read the increments)
    if (lane == 0) {
      C.st = st;
      const size_t ix = (size_t)k * (size_t)a.n + (size_t)e;
      if (a.dice) {
        a.dice[2 * ix] = (uint8_t)d0;
        a.dice[2 * ix + 1] = (uint8_t)d1;
      }
      if (a.actions) reinterpret_cast<uint32_t*>(a.actions)[ix] = pack_codes(o.code1, o.code2);
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

// k_turn_value_rollout's ply loop likewise: a wave takes each env's pair when
// it starts that env
template <bool kRec>
__global__ void __launch_bounds__(64) k_turn_value_rollout_league(TvrArgs a, LeagueArgs lg) {
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
    const int iw = (int)vr_uniform((uint32_t)lg.white[e]), ib = (int)vr_uniform((uint32_t)lg.black[e]);
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
      const int idx = black ? ib : iw;
      const bool has = (uint32_t)idx < (uint32_t)lg.n_nets;
      RowBest b = row_best_none();
      uint64_t pw = ~0ull;  // no row: the all -1 play
      if (has) {            // wave-uniform
        const ValNet vn = league_net(lg.table, idx);
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
      else  // narde_step_full(play = NULL)'s own turn, as k_turn_value_rollout plays it
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
