// kernels_league.h -- round-robin leagues in one launch: a value net per env and colour
// Part of the one translation unit narde.hip (included there, in order, last:
// the plies and the envs' loops -- vr_ply and vr_env_plies, tvr_ply and
// tvr_env_plies -- are kernels_value_rollout.h's and
// kernels_turn_value_rollout.h's; this file adds the table and the net source
// that reads it); not a standalone header.
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

// The plies' net source (VrTwoNets' interface) of env e: its pair is read
// once, here; the mover's entry once a ply, inside the plies' `if (has)`
struct LeagueNets {
  const LeagueNet* __restrict__ table;
  int n_nets, iw, ib;
  __device__ __forceinline__ bool has(bool black) const { return (uint32_t)(black ? ib : iw) < (uint32_t)n_nets; }
  __device__ __forceinline__ ValNet net(bool black) const { return league_net(table, black ? ib : iw); }
};
__device__ __forceinline__ LeagueNets league_nets(const LeagueArgs& lg, int e) {
  return LeagueNets{lg.table, lg.n_nets, (int)vr_uniform((uint32_t)lg.white[e]), (int)vr_uniform((uint32_t)lg.black[e])};
}

// k_value_rollout with the env's nets taken from the table
template <bool kRec>
__global__ void __launch_bounds__(64) k_value_rollout_league(VrArgs a, LeagueArgs lg) {
  __shared__ AftScan L;
  __shared__ ValStage VS;
  __shared__ VrStage CS;
  __shared__ VrCarry C;
  const int e = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  if (e >= a.n) return;
  vr_env_plies<kRec>(a, e, league_nets(lg, e), L, VS, CS, C, threadIdx.x & 63);
}

// k_turn_value_rollout likewise: a wave takes each env's pair when it starts
// that env
template <bool kRec>
__global__ void __launch_bounds__(64) k_turn_value_rollout_league(TvrArgs a, LeagueArgs lg) {
  __shared__ TurnFrontLds F;
  __shared__ TurnScan L;
  __shared__ ValStage VS;
  __shared__ VrCarry C;
  const int wave = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const TurnSlab slab = turn_slab(a.slab, wave);
  for (int e = wave; e < a.n; e += (int)gridDim.x)
    tvr_env_plies<kRec>(a, e, league_nets(lg, e), slab, F, L, VS, C, threadIdx.x & 63);
}

}  // namespace
