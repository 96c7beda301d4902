// kernels_turn_value_playout.h -- Monte-Carlo playouts of given FULL4 positions under value nets
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_turn_value_rollout.h and kernels_value_playout.h: the ply is
// tvr_ply of the former, VpArgs, vp_leaf and vp_store are the latter's); not a
// standalone header.
#pragma once

namespace {

// one-wave workgroups; wave w plays trials w, w + gridDim.x, ... (static: the
// bits do not depend on the number of waves), each from its root's record to
// the first terminal ply or max_plies, whole turns (tvr_ply with the call's
// own Rng, no explore draw, max_steps 0, no auto-reset and no statistics)
__global__ void __launch_bounds__(64) k_turn_value_playout(VpArgs a, ValNet net_w, ValNet net_b, int has_w,
                                                           int has_b) {
  __shared__ TurnFrontLds F;
  __shared__ TurnScan L;
  __shared__ ValStage VS;
  __shared__ VrCarry C;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const int waves = (int)gridDim.x;
  const TurnSlab slab = turn_slab(a.slab, wave);
  const VrTwoNets nets{net_w, net_b, has_w, has_b};
  const int total = a.n * a.trials;
  for (int q = wave; q < total; q += waves) {
    const int root = q / a.trials;
    const int e = a.common ? q - root * a.trials : q;  // the trial's env index in the ply stream
    Side s = side_from_record(a.roots[2 * (size_t)root], a.roots[2 * (size_t)root + 1]);
    wave_lds_handoff();  // (the last trial's reads of the carry are done)
    int done = 0, outc = 0, len = 0;
    for (int k = 0; k < a.max_plies; ++k) {
      const TvrPly p = tvr_ply<false>(s, a.g, e, k, nets, VrExplore{}, 0, false, slab, F, L, VS, C, lane);
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
}

}  // namespace
