// kernels_turn_value_playout.h -- Monte-Carlo playouts of given FULL4 positions under value nets
// Part of the one translation unit narde.hip (included there, in order,
// behind kernels_turn_value_rollout.h and kernels_value_playout.h: the ply is
// k_turn_value_rollout's, turn_pick_roll, VpArgs, vp_leaf and vp_store are
// there); not a standalone header.
#pragma once

namespace {

// one-wave workgroups; wave w plays trials w, w + gridDim.x, ... (static: the
// bits do not depend on the number of waves), each from its root's record to
// the first terminal ply or max_plies, whole turns (k_turn_value_rollout's ply
// with the call's own Rng, max_steps 0 and no auto-reset)
__global__ void __launch_bounds__(64) k_turn_value_playout(VpArgs a, ValNet net_w, ValNet net_b, int has_w,
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
  const int total = a.n * a.trials;
  for (int q = wave; q < total; q += waves) {
    const int root = q / a.trials;
    const int e = a.common ? q - root * a.trials : q;  // the trial's env index in the ply stream
    Side s = side_from_record(a.roots[2 * (size_t)root], a.roots[2 * (size_t)root + 1]);
    wave_lds_handoff();  // (the last trial's reads of the carry are done)
    int done = 0, outc = 0, len = 0;
    for (int k = 0; k < a.max_plies; ++k) {
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
      uint64_t pw = ~0ull;  // no row: the all -1 play
      if (has) {            // wave-uniform
        const ValNet vn = vr_net(black, net_w, net_b);
        // the values are white's: black plays the smallest
        TurnPick pk{{s, d0, d1, nullptr, black, 0.0f}, false, 0u, row_best_none(), 0, 0, 0};
        wave_lds_handoff();  // the last ply's reads of the frontier are done
        int nrows = turn_pick_roll(pk, F.key, F.path[0], F.path[1], kTurnFront, L, vn, VS);
        if (nrows < 0) {  // wave-uniform: the same walk in the wave's piece of the slab
          wave_lds_handoff();
          nrows = turn_pick_roll(pk, skey, spathA, spathB, kTurnAftMax, L, vn, VS);
        }
        if (nrows > 0) pw = turn_path_play_words(pk.b.codes, pk.level, pk.dh, pk.dl);
      }
      wave_lds_handoff();  // lane 0's block, to every lane
      uint32_t R[4], r[4];
      vr_load4(C.R, R);
      ply_words_of(R, s.t, a.g.dice_mode, r);
      int4 st = make_int4(0, 0, 0, 0);
      TurnOut o;
      int term, trunc;
      if (has)  // wave-uniform
        env_ply_full(s, st, r, a.g.env0 + (uint32_t)e, a.g.k0, a.g.k1, false, 0, 0, a.g.dice_mode, true, pw, 0, false, o,
                     term, trunc);
      else  // narde_step_full(play = NULL)'s own turn
        ply_full_words(s, st, r, a.g.dice_mode, 0, false, o, term, trunc);
      wave_lds_handoff();  // (every lane has read the block)
      len = k + 1;
      if (vr_uniform((uint32_t)term) != 0u) {  // wave-uniform: the trial ends here
        done = 1;
        outc = (int)vr_uniform((uint32_t)(black ? -o.reward : o.reward));
        break;
      }
    }
    float leaf = __builtin_nanf("");
    if (a.leaf && !done) leaf = vp_leaf(s, net_w, net_b, has_w, has_b, VS, lane);
    vp_store(a, q, root, lane, done, outc, len, leaf);
  }
}

}  // namespace
