// kernels_value_playout.h -- Monte-Carlo playouts of given positions under value nets
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_value_rollout.h and kernels_turn_value_rollout.h: the ply is
// vr_ply there, as are vr_net, vr_uniform and the carry); not a standalone
// header.
#pragma once

namespace {

// narde_state_records: k_set_state's packing into a caller's records
// [n][2] (p0 then p1 of a position), the ply counter t, elapsed 0.
__global__ void __launch_bounds__(kBlock) k_state_records(int64_t n, const int8_t* __restrict__ board,
                                                          const uint8_t* __restrict__ off,
                                                          const uint8_t* __restrict__ ft,
                                                          const int8_t* __restrict__ player, uint32_t t,
                                                          uint4* __restrict__ records) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint4 a, b;
  record_from_board(board + (size_t)i * 24, off[2 * i], off[2 * i + 1], ft[2 * i], ft[2 * i + 1], player[i], 0u, t, a,
                    b);
  records[2 * i] = a;
  records[2 * i + 1] = b;
}

// the sums' zeros ahead of the trials' atomic adds
__global__ void __launch_bounds__(kBlock) k_playout_zero(int32_t* __restrict__ sums, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) sums[i] = 0;
}

// narde_value_playout / narde_turn_value_playout: trial j of root i, local
// index q = i * trials + j, plays from roots[i] the plies the value rollout
// plays for an env with that record at env index q (common dice: j) of a
// handle with env0 = g.env0, max_steps 0 -- with no auto-reset, until the
// first terminal ply or max_plies.  Nothing of a handle is read or written.
struct VpArgs {
  const uint4* __restrict__ roots;  // [n][2]
  int n, trials, max_plies;
  Rng g;       // the call's own: env0 = id_base, the key from seed, the handle's dice law
  int common;  // NARDE_PLAYOUT_COMMON_DICE: trial j's env index is j for every root
  int32_t* __restrict__ sums;     // [n][4], zeroed ahead of the launch
  int8_t* __restrict__ outcome;   // [n][trials]
  int32_t* __restrict__ length;   // [n][trials]
  float* __restrict__ leaf;       // [n][trials]
  uint8_t* __restrict__ slab;     // FULL4: [gridDim.x][kTurnSlabWave]
};

// white's value of s under vn by the whole wave: the root forward of the
// scored rows (val_root) and the second layer on it, the same in every lane
__device__ __forceinline__ float vp_leaf_value(const Side& s, const ValNet& vn, ValStage& VS, int lane) {
  uint4 ra, rb;
  side_to_record(s, ra, rb);
  ValRoot vr;
  val_root(vr, vn, VS, ra, rb, lane);
  float v = 0.0f;
  val_units(vr.nu, [&](auto NU) {
    float part = val_lane_part<NU.value>(vr.z, vr.w2, vn.hidden_act);
#pragma unroll
    for (int o = kValLanes / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    v = val_out_act(vr.b2 + part, vn.out_act);
  });
  return v;
}

// trial q's results, from lanes 0..3: the per-trial arrays and the root's four
// sums (integer vector atomics: the same bits in any order)
__device__ __forceinline__ void vp_store(const VpArgs& a, int q, int root, int lane, int done, int outc, int len,
                                         float leaf) {
  if (lane < 4) {
    const int v = lane == 0 ? done : (lane == 1 ? outc : (lane == 2 ? outc * outc : len));
    atomicAdd(a.sums + 4 * (size_t)root + lane, v);
  }
  if (lane == 0) {
    if (a.outcome) a.outcome[q] = (int8_t)outc;
    if (a.length) a.length[q] = len;
    if (a.leaf) a.leaf[q] = leaf;
  }
}

// the record a trial stopped at, unfinished: its mover's net, or the other
// colour's if the mover has none
__device__ __forceinline__ float vp_leaf(const Side& s, const ValNet& net_w, const ValNet& net_b, int has_w, int has_b,
                                         ValStage& VS, int lane) {
  const bool black = vr_uniform(s.black) != 0u;
  const bool use_b = black ? has_b != 0 : has_w == 0;
  return vp_leaf_value(s, vr_net(use_b, net_w, net_b), VS, lane);
}

// one wave per trial, a trial per workgroup (k_value_rollout's LDS)
__global__ void __launch_bounds__(64) k_value_playout(VpArgs a, ValNet net_w, ValNet net_b, int has_w, int has_b) {
  __shared__ AftScan L;
  __shared__ ValStage VS;
  __shared__ VrStage CS;
  __shared__ VrCarry C;
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  if (q >= a.n * a.trials) return;
  const int root = q / a.trials;
  const int e = a.common ? q - root * a.trials : q;  // the trial's env index in the ply stream
  Side s = side_from_record(a.roots[2 * (size_t)root], a.roots[2 * (size_t)root + 1]);
  int done = 0, outc = 0, len = 0;
  const VrTwoNets nets{net_w, net_b, has_w, has_b};
  for (int k = 0; k < a.max_plies; ++k) {  // greedy plies, max_steps 0, no auto-reset, no statistics
    const VrPly p = vr_ply<false>(s, a.g, e, k, nets, VrExplore{}, 0, false, L, VS, CS, C, lane);
    len = k + 1;
    if (vr_uniform((uint32_t)p.term) != 0u) {  // wave-uniform: the trial ends here
      done = 1;
      outc = (int)vr_uniform((uint32_t)(p.black ? -p.o.reward : p.o.reward));
      break;
    }
  }
  float leaf = __builtin_nanf("");
  if (a.leaf && !done) leaf = vp_leaf(s, net_w, net_b, has_w, has_b, VS, lane);
  vp_store(a, q, root, lane, done, outc, len, leaf);
}

}  // namespace
