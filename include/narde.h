/*
 * narde.h -- C ABI of libnarde, the MI355X-native batched Narde environment.
 *
 * The reference (dmytroleonenko/gym-narde) is pure Python and has no FFI;
 * this ABI is the boundary UNDER a Python facade that reproduces its
 * gymnasium surface (gym-narde_amd/gym_narde/).  Each entry point names the
 * reference function it replaces (paths under the reference checkout):
 *
 *   narde_reset              NardeEnv.reset           gym_narde/envs/narde_env.py:105-120
 *   narde_legal_moves        Narde.get_valid_moves    gym_narde/envs/narde.py:58-92
 *   narde_step               NardeEnv.step            gym_narde/envs/narde_env.py:27-103
 *   narde_apply_moves        Narde.execute_rotated_move gym_narde/envs/narde.py:36-56
 *   narde_violates_block_rule Narde._violates_block_rule gym_narde/envs/narde.py:139-184
 *   narde_observe            NardeEnv._get_obs / get_perspective_board
 *                                                     gym_narde/envs/narde_env.py:24-25,
 *                                                     gym_narde/envs/narde.py:31-34
 *                            + 198-float Tesauro obs   README.md:42-102 (spec only)
 *   narde_get/set_state      direct `env.unwrapped.game` attribute access
 *                            (train_deepq_pytorch.py:867-931, evaluate_model.py:22-134)
 *   narde_selfplay           random-policy self-play loop (no reference equivalent;
 *                            the benchmark workload of BASELINE.json)
 *   narde_host_*             the same rules on small HOST batches (the scalar
 *                            gym facade): staged through pinned memory, synchronous.
 *
 * Conventions
 *   - Every pointer argument of a non-host entry point is a DEVICE pointer on
 *     the handle's device (e.g. a torch tensor's data_ptr()); NULL means
 *     "not requested" where documented.  Arrays are C-contiguous.
 *   - `stream` is a hipStream_t (NULL = the null stream).  Calls are stream-
 *     ordered and never synchronise unless documented (narde_host_*).
 *   - Board layout = the reference's: int8[24] absolute points, white > 0,
 *     black < 0 (point p = index p, white head 23, black head 11).
 *     off = {borne_off_white, borne_off_black}; first_turn = {white, black};
 *     player = current mover, +1 white / -1 black.
 *   - A move is (from, to) in the MOVER's perspective, to = 24 for 'off'.
 *   - Action codes are the reference's: from*24 + to, with to == 0 and
 *     from <= 5 meaning (from, 'off') (narde_env.py:238-254).
 *   - Return value: 0 on success, negative NARDE_E* on error;
 *     narde_last_error() gives a message (thread-local).
 */
#ifndef NARDE_H
#define NARDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NARDE_OK 0
#define NARDE_EINVAL (-1)
#define NARDE_EHIP (-2)
#define NARDE_ENOMEM (-3)

#define NARDE_DICE_ALL36 0      /* dice uniform over the 36 ordered pairs      */
#define NARDE_DICE_NODOUBLES 1  /* uniform over the 30 non-double ordered pairs */

#define NARDE_MAX_MOVES 64      /* list capacity per env (4-die rolls give <= 60) */
#define NARDE_OFF 24

typedef struct narde_env narde_env; /* B envs resident in HBM on one device */

int narde_version(void);
const char *narde_last_error(void);

/* Allocate B = num_envs env records on `device`.  Global env ids are
 * env_id_offset .. env_id_offset+B-1 (device RNG is keyed by the global id,
 * so a sharded run reproduces a single-GPU run).  max_episode_steps is the
 * gymnasium TimeLimit (reference registers 1000: gym_narde/__init__.py:3-7);
 * 0 disables truncation.  Envs start in the reset state of epoch 0. */
int narde_create(int device, int64_t num_envs, int64_t env_id_offset, uint64_t seed,
                 int dice_mode, int max_episode_steps, narde_env **out);
int narde_destroy(narde_env *env);
int64_t narde_num_envs(const narde_env *env);
/* Per-env RNG ply counter t (kept in the env record, +1 per step, kept
 * across episodes): the device dice/policy draws of an env's next step are
 * Philox4x32-10(ctr = {t, global_env_id, 0, 0}, key = seed).  Because t lives
 * in device state, narde_step / narde_rollout launches can be captured in a
 * hipGraph and replayed.  get_ply reads env 0's counter and set_ply sets
 * every env's counter; both synchronise the whole device first
 * (hipDeviceSynchronize), so work queued on any stream is ordered before
 * them -- a device-wide barrier: they also wait for every other stream of
 * the process on that device, unrelated work (training, other handles)
 * included.  Neither belongs in a hot loop. */
int narde_get_ply(const narde_env *env, uint32_t *t);
int narde_set_ply(narde_env *env, uint32_t t);

/* NardeEnv.reset: start position + opening roll.  mask[B] (u8) selects envs,
 * NULL = all.  opening (optional) u8[B][pairs][2]: each env's opening draws
 * (white roll, black roll) in the order the reference draws them
 * (narde_env.py:111-117): the first pair of different dice decides, the
 * higher roll moves first; pairs with a die outside 1..6 are padding, and an
 * env whose row has no deciding pair (or opening = NULL) takes the device
 * draw, uniform over the 30 unequal ordered pairs.  Zeroes the per-env
 * statistics of reset envs. */
int narde_reset(narde_env *env, const uint8_t *mask, const uint8_t *opening, int pairs,
                void *stream);

/* Direct state access.  elapsed may be NULL (set: 0).  The device path does
 * NOT validate: a board value outside [-15, 15], more than 15 checkers (on
 * the board + off) of a colour, off > 15 or a player other than +1/-1 wraps
 * into neighbouring 4-bit fields of the record, so callers must pass legal
 * positions.  The narde_host_* entry points check every position and return
 * NARDE_EINVAL instead. */
int narde_set_state(narde_env *env, const int8_t *board, const uint8_t *off,
                    const uint8_t *first_turn, const int8_t *player, const uint16_t *elapsed,
                    void *stream);
int narde_get_state(narde_env *env, int8_t *board, uint8_t *off, uint8_t *first_turn,
                    int8_t *player, uint16_t *elapsed, void *stream);

/* Dice the next narde_step(dice = NULL) will use, in roll order: u8[B][2]. */
int narde_peek_dice(narde_env *env, uint8_t *dice, void *stream);

/* Narde.get_valid_moves(roll, current_player) for every env's mover.
 * dice: u8[B][4], 1..4 dice per env, unused slots 0; NULL = the next step's
 * device dice.  out_count: i16[B].  out_moves (optional): i8[B][64][2] (from,
 * to), -1 padded, exactly the reference's list (order + duplicates).
 * out_compact (optional, only for <= 2 dice): u64[B] = L_hi | L_lo<<24 |
 * d_hi<<48 | d_lo<<52 where L_* are the per-die 24-bit source masks. */
int narde_legal_moves(narde_env *env, const uint8_t *dice, int16_t *out_count,
                      int8_t *out_moves, uint64_t *out_compact, void *stream);

/* NardeEnv.step for all B envs.  actions i16[B][2] = (move1_code,
 * move2_code); NULL = in-kernel random legal policy.  dice u8[B][2] in roll
 * order; NULL = device RNG at each env's counter t.  A given die outside 1..6
 * makes that env's ply one with no legal move (list #1 empty: no checker
 * moves, the player changes, t and the TimeLimit count advance); the same
 * holds for the given dice of narde_step_full / narde_legal_full /
 * narde_legal_mask576_move2 (no sub-move / legal word 0 / empty mask).  Outputs (each optional, NULL = skip):
 * obs i32[B][24] (next mover's perspective), reward i32[B], terminated u8[B],
 * truncated u8[B], legal_compact u64[B] (list #1, format above),
 * actions_out i16[B][2] (codes actually used).  autoreset != 0: envs that
 * terminate or truncate are reset in the same call (obs is then the new
 * episode's first obs) and counted in the statistics.  Increments every
 * env's t. */
int narde_step(narde_env *env, const int16_t *actions, const uint8_t *dice, int32_t *obs,
               int32_t *reward, uint8_t *terminated, uint8_t *truncated,
               uint64_t *legal_compact, int16_t *actions_out, int autoreset, void *stream);

/* `plies` plies of random-legal self-play with auto-reset in ONE launch, the
 * env record kept in registers across plies.  Every ply's outputs are
 * streamed to rollout buffers laid out [plies][B][...] with the per-ply
 * formats of narde_step (each optional, NULL = skip).  Statistics accumulate
 * as in narde_step.  Equivalent to `plies` narde_step(actions = NULL,
 * dice = NULL, autoreset = 1) calls. */
int narde_rollout(narde_env *env, int plies, int32_t *obs, int32_t *reward, uint8_t *terminated,
                  uint8_t *truncated, uint64_t *legal_compact, int16_t *actions_out, void *stream);

/* narde_rollout with no per-ply outputs (statistics only). */
int narde_selfplay(narde_env *env, int plies, void *stream);

/* ---- FULL4 rules mode (build extension) -------------
 * One step = the mover's WHOLE turn: four sub-moves on doubles, the
 * max-dice-used rule, the higher die when only one of two dice can be used,
 * at most one checker off the head per turn (two on a first-turn 3-3, 4-4 or
 * 6-6).  Every sub-move is the reference's single-die primitive
 * (Narde.get_valid_moves([die]) narde.py:58-92, execute_rotated_move
 * narde.py:36-56); the reference env itself stops after two checker moves
 * (narde_env.py:45-93), so whole-turn parity is against the build's oracle,
 * which is pinned sub-move by sub-move to the reference (tests/golden/full4.npz).
 * A sub-move is (from, die), from in the mover's perspective; the landing
 * point is from - die, or 'off' when negative.
 *   legal_first u64[B] = C_hi | C_lo<<24 | d_hi<<48 | d_lo<<52 | M<<56: the
 *     sources playable as the FIRST sub-move with the higher / lower die
 *     (doubles: C_lo = 0, d_lo = d_hi) and M = max dice usable (0..4).
 *   played u64[B]: bytes 2k / 2k+1 = from / die of sub-move k, 0xFF unused.
 *   play i8[B][4][2] (from, die): applied while each sub-move keeps M
 *     reachable; the first one that does not ends the turn (illegal actions
 *     are ignored, as in narde_env.py:56-93).  NULL = in-kernel random policy
 *     (sub-move k uniform over its legal set). */
int narde_step_full(narde_env *env, const int8_t *play, const uint8_t *dice, int32_t *obs,
                    int32_t *reward, uint8_t *terminated, uint8_t *truncated,
                    uint64_t *legal_first, uint64_t *played, int autoreset, void *stream);
/* `plies` FULL4 random-policy turns per env in ONE launch (outputs [plies][B]). */
int narde_rollout_full(narde_env *env, int plies, int32_t *obs, int32_t *reward,
                       uint8_t *terminated, uint8_t *truncated, uint64_t *legal_first,
                       uint64_t *played, void *stream);
int narde_selfplay_full(narde_env *env, int plies, void *stream);
/* narde_rollout (full = 0; `last` = actions i16[plies][B][2]) or
 * narde_rollout_full (full = 1; `last` = played u64[plies][B]) with HIP
 * events recorded on `stream` just before the launch (ev_start) and just
 * after it (ev_stop), each optional (NULL): a timed launch is one call
 * instead of three (bench.py's timed region).  totals (optional): the
 * launch also writes the statistics of narde_get_stats after it, summed per
 * workgroup of 256 envs, as i64[NARDE_WG_ROWS(B)][3] {episodes, white
 * points, black points} (row r: envs 256 r .. 256 r + 255) -- the self-play
 * driver's per-run result with no second launch.  plies = 0 launches
 * nothing (and then totals must be NULL). */
#define NARDE_WG_ROWS(num_envs) (((num_envs) + 255) / 256)
int narde_rollout_timed(narde_env *env, int full, int plies, int32_t *obs, int32_t *reward,
                        uint8_t *terminated, uint8_t *truncated, uint64_t *legal, void *last,
                        void *ev_start, void *ev_stop, int64_t *totals, void *stream);
/* narde_rollout_timed pre-bound (round 6): _create checks the arguments,
 * chooses the kernel and packs its arguments once (plies > 0; the calling
 * thread's current device must be the env's); _launch then records ev_start,
 * launches and records ev_stop on `stream` -- the same launch as
 * narde_rollout_timed with the same arguments, one pointer per call (the
 * caller keeps the thread's current device and every buffer as at create);
 * _destroy frees the plan (host memory only). */
int narde_rollout_plan_create(narde_env *env, int full, int plies, int32_t *obs, int32_t *reward,
                              uint8_t *terminated, uint8_t *truncated, uint64_t *legal,
                              void *last, void *ev_start, void *ev_stop, int64_t *totals,
                              void *stream, void **plan);
int narde_rollout_plan_launch(void *plan);
int narde_rollout_plan_destroy(void *plan);
/* Timing events for narde_rollout_timed on `device`: a HIP event (returned
 * as void*) created with hipEventCreateWithFlags(flags); flags 0 = HIP's
 * default, 0x20000000 = hipEventDisableSystemFence (the event's record does
 * no system-scope cache write-back / invalidate: a timing-only marker, what
 * bench.py uses).  elapsed_ms = hipEventElapsedTime (both recorded and
 * complete). */
int narde_timing_event_create(int device, unsigned flags, void **event);
int narde_timing_event_destroy(void *event);
int narde_timing_event_elapsed_ms(void *start, void *stop, float *ms);
/* C_0 and M for dice u8[B][2] (NULL = the next step's device dice). */
int narde_legal_full(narde_env *env, const uint8_t *dice, uint64_t *legal_first, void *stream);

/* Per-env statistics i32[B][3] = {episodes finished, white points, black
 * points} since the last reset of that env. */
int narde_get_stats(narde_env *env, int32_t *stats, void *stream);

/* The same statistics summed over the handle's envs, as NARDE_TOTAL_ROWS
 * partial rows i64[NARDE_TOTAL_ROWS][3] (row b: the b-th contiguous range
 * of envs); the totals are the column sums.  One launch -- what a sharded
 * self-play run all-gathers per rank (the reference's returns, collected
 * by its training loops: train_deepq_pytorch.py:855-1081). */
#define NARDE_TOTAL_ROWS 64
int narde_get_totals(narde_env *env, int64_t *rows, void *stream);

/* execute_rotated_move(move, player) per env: moves i8[B][2] in the
 * perspective of player[B] (+1/-1; NULL = each env's current mover);
 * from < 0 skips the env.  Clears that player's first_turn flag.  A move the
 * record cannot hold -- the source has none of the player's checkers, or the
 * target holds opponent checkers (the reference, narde.py:108-125, would
 * conjure or cancel checkers) -- leaves that env unchanged; every listed move
 * is executable.  narde_host_apply_moves returns NARDE_EINVAL for one. */
int narde_apply_moves(narde_env *env, const int8_t *moves, const int8_t *player, void *stream);

/* obs i32[B][24] (current mover's perspective) and/or the 198-float
 * Tesauro observation f32[B][198] (absolute points; white block first). */
int narde_observe(narde_env *env, int32_t *obs, float *tesauro198, void *stream);

/* 576-bit mask of legal move1 action codes for the next step's dice:
 * u64[B][9], bit c set iff the reference would accept code c as move1. */
int narde_legal_mask576(narde_env *env, uint64_t *mask, void *stream);

/* Move-2 acceptance mask u64[B][9] given each env's move-1 code i16[B] and
 * dice u8[B][2] in roll order (NULL = the next step's device dice): bit c
 * set iff NardeEnv.step would play code c as move2 after move1
 * (narde_env.py:56-93); all zero when move1 would not be played.  With
 * narde_legal_mask576 it gives a policy the exact legal set of (move1,
 * move2) codes (train_deepq_pytorch.py:411-600 approximates it). */
int narde_legal_mask576_move2(narde_env *env, const int16_t *move1, const uint8_t *dice,
                              uint64_t *mask, void *stream);

/* The plays of each env's two-dice roll (the README's get_valid_actions,
 * README.md:156-165), for dice u8[B][2] in roll order (NULL = the next
 * step's device dice).  Replaces the per-env Python lists of
 * DQNAgent.act (train_deepq_pytorch.py:430-507, kind 0) and the (m1, m2)
 * set NardeEnv.step carries out (narde_env.py:45-93, kind 1; the facade's
 * Narde.get_valid_plays).  Outputs: legal u64[B] (optional) = list #1 in
 * the compact format above; table u32[B][2][24]: for each list-#1 entry
 * (k = 0 the higher die's list, k = 1 the lower's; source p) the word
 * second-move sources (24 bits) | rem << 24 | 1 << 27, 0 where (k, p) is no
 * entry -- kind 0: rem = the roll less the die act() matches to move 1
 * (exact distance in roll order; a bear-off from p: the first die >= p+1),
 * its list get_valid_moves([rem]) on the pre-move board; kind 1: move 1
 * applied, rem per the step's bookkeeping, list #2 on the post-move board
 * (a one-entry list #1: word 1 << 27, played alone); count i32[B]: kind 0
 * len(valid_move_combinations) (every entry, duplicates included, times
 * max(1, |its list|)), kind 1 the number of distinct plays.  A die outside
 * 1..6: list 0, count 0. */
int narde_play_set(narde_env *env, const uint8_t *dice, int kind, uint64_t *legal, uint32_t *table,
                   int32_t *count, void *stream);

/* DQNAgent.act's greedy candidate sets (train_deepq_pytorch.py:520-560) as
 * 576-bit masks u64[B][9], for dice u8[B][2] in roll order (NULL = the next
 * step's device dice).  move1 NULL: bit c set iff c is the code act() gives
 * some list-#1 entry (valid_first_moves' keys).  move1 int64 (element i at
 * move1[i * ld_move1]): the move-2 codes act() offers after move 1 --
 * valid_first_moves[move1]: the pre-move second list of the LAST list-#1
 * entry with that code, bit 0 alone if that list is empty, no bit if no
 * entry has that code. */
int narde_act_masks(narde_env *env, const uint8_t *dice, const int64_t *move1, int64_t ld_move1,
                    uint64_t *mask, void *stream);

/* The DQN driver's exploration (train_deepq_pytorch.py:514-515): for the
 * rows whose explore draw Philox4x32-10({*tag, row, 0, 5}, seed) r0 <
 * *epsilon * 2^32 (the policy kernels' shared decision), writes play
 * mulhi(r1, count) of act()'s combination list (kind 0 above: uniform over
 * (move1, move2) combinations) into out[row * ld_out + 0..1] (int64 codes);
 * other rows, and rows with no play, are left untouched.  dice as above. */
int narde_explore_plays(narde_env *env, const uint8_t *dice, const float *epsilon, uint64_t seed,
                        const int64_t *tag, int64_t *out, int64_t ld_out, void *stream);

/* Afterstates: the successor positions of each env's two-dice roll (REF2),
 * what a TD-Gammon value network scores (README.md:42-102 the 198-float
 * encoding, README.md:156-165 get_valid_actions).  dice u8[B][2] in roll
 * order (NULL = the next step's device dice).  Per env, the plays
 * NardeEnv.step carries out (narde_env.py:27-103; narde_play_set kind 1) in
 * list order -- list #1's entries in list order, duplicate entries skipped,
 * the second-move sources ascending; an entry with no second move, or a
 * one-entry list #1, is a one-move play -- keeping only plays whose moves
 * action codes express (decode(encode(f, t)) == (f, t): not a normal move
 * landing on point 0 from 1..5; a one-entry list #1 is played whatever the
 * action and always kept), each carried out as narde_step(actions = (c1,
 * c2), dice, autoreset = 0) does, and of the plays that leave the same board
 * and off counts only the first.  Rows are CSR: env e's rows are
 * offsets[e] .. offsets[e + 1] - 1 (offsets i32[B + 1], offsets[0] = 0), in
 * that order, the same on every call (no atomics).  A die outside 1..6 or no
 * expressible play: no row.  Per row (every array optional, NULL = not
 * wanted): row_env i32 = e; codes i16[2] = (c1, c2), c2 = 0 for a one-move
 * play; feat f32[198] = narde_observe's tesauro198 after that step (the
 * mover is not flipped after a terminal step); obs i32[24] and reward i8 =
 * that step's outputs (reward != 0 = terminated).  cap = rows the arrays
 * hold: rows >= cap are not written and nothing past cap rows is touched;
 * offsets always holds the true counts, so offsets[B] > cap tells the caller
 * it overflowed.  cap = 0 with every row array NULL counts only.  feat and
 * obs must be 16-byte aligned.  Stream-ordered, no allocation, no
 * synchronise: graph-capturable.  B x 1152 must stay below 2^31. */
int narde_afterstates(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                      int32_t *row_env, int16_t *codes, float *feat, int32_t *obs, int8_t *reward,
                      void *stream);

/* Value-greedy play over narde_afterstates' rows: one row per env from
 * value[r * ld_value] (a value network's output for feat row r).
 * perspective 0: the values are the mover's -- the largest; perspective 1:
 * they are white's (the README's reward, "+1 if WHITE wins") -- the largest
 * when white moves, the smallest when black does (read from the record, so
 * call it before the step).  The lowest row on ties; a NaN as torch.max /
 * torch.min(dim) take it.  Rows >= cap are ignored.  epsilon f32 / tag i64
 * device scalars (epsilon NULL = greedy): when the env's explore draw
 * Philox4x32-10({*tag, env, 0, 5}, seed) r0 < *epsilon * 2^32, the row is
 * offsets[e] + mulhi(r1, count) instead.  actions i16[B][2] = the row's
 * codes, ready for narde_step; row i32[B] (optional) = the row, -1 and
 * actions (0, 0) for an env with no row. */
int narde_afterstate_pick(narde_env *env, const int32_t *offsets, const int16_t *codes, int64_t cap,
                          const float *value, int64_t ld_value, int perspective, const float *epsilon,
                          uint64_t seed, const int64_t *tag, int16_t *actions, int32_t *row,
                          void *stream);

/* FULL4 whole-turn afterstates: the distinct positions a whole turn can
 * leave (four sub-moves on doubles, the max-dice-used rule), stated against
 * or_full4_turn (oracle/narde_oracle.c).  A play is a sequence of sub-moves
 * (from, die), each taken from C_k for the prefix before it, of length M;
 * plays are ordered lexicographically, each sub-move in list order (higher
 * die first, source ascending).  A play's afterstate is what
 * narde_step_full(play, dice, autoreset = 0) leaves: the sub-moves, then
 * _check_game_ended and the flip (the mover is not flipped after a terminal
 * turn).  An env's rows are its DISTINCT afterstates (equal board and off
 * counts are the same), ordered by the first play that produces each one;
 * that play is the row's.  The order is the same on every call (no atomic
 * decides it).  M = 0 (a pass) or a die outside 1..6: no row.  The result is
 * exact for every position: a row count per env never exceeds
 * NARDE_TURN_AFT_MAX (DESIGN.md section 14.2 derives it) and none is
 * truncated.
 * offsets i32[B + 1] CSR as narde_afterstates.  Per row (every array
 * optional): row_env i32; play i8[4][2] = (from, die), -1 padding, ready for
 * narde_step_full; feat f32[198] = narde_observe's tesauro198 after that
 * turn; obs i32[24]; reward i8 (!= 0 = terminated).  cap clamps what is
 * written, never what offsets holds; nothing past cap rows is touched;
 * cap = 0 with every row array NULL counts only.  dice NULL = the next
 * step's device dice.  feat and obs 16-byte, play 8-byte aligned.
 * Stream-ordered, no synchronise, graph-capturable; the handle's workspace
 * (11 MB) is allocated by the handle's first call, which must be made
 * outside capture.  B x NARDE_TURN_AFT_MAX must stay below 2^31. */
#define NARDE_TURN_AFT_MAX 5220
int narde_turn_afterstates(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                           int32_t *row_env, int8_t *play, float *feat, int32_t *obs, int8_t *reward,
                           void *stream);

/* narde_afterstate_pick over narde_turn_afterstates' rows (the same
 * perspective, tie, NaN and explore-draw rules; one shared selection):
 * out_play i8[B][4][2] = the row's play, all -1 for an env with no row,
 * ready for narde_step_full; row i32[B] (optional).  play and out_play
 * 8-byte aligned. */
int narde_turn_pick(narde_env *env, const int32_t *offsets, const int8_t *play, int64_t cap,
                    const float *value, int64_t ld_value, int perspective, const float *epsilon,
                    uint64_t seed, const int64_t *tag, int8_t *out_play, int32_t *row, void *stream);

/* Afterstates scored by a built-in value MLP:
 *   v(row) = g_out(b2 + sum_h w2[h] g_hid(b1[h] + sum_c feat[c] W1[h][c]))
 * over the row's tesauro198 columns feat, which are never written: the fill
 * pass evaluates the first layer as the env's own pre-activations plus the
 * few columns in which the row differs from it, and stores one float a row.
 * Every pointer of narde_value_mlp is device memory, read when the kernels
 * run -- weights changed between two replays of a captured graph are seen by
 * the second.  w1t is feature-major: w1t[c * ld_w1t + h] = W1[h][c]. */
#define NARDE_VALUE_HIDDEN_MAX 128
typedef struct narde_value_mlp {
  const float *w1t;    /* f32[198][ld_w1t] */
  int64_t ld_w1t;      /* >= hidden */
  const float *b1;     /* f32[hidden] */
  const float *w2;     /* f32[hidden] */
  const float *b2;     /* f32[1] */
  int32_t hidden;      /* 1 .. NARDE_VALUE_HIDDEN_MAX */
  int32_t hidden_act;  /* 0 sigmoid, 1 tanh, 2 relu */
  int32_t out_act;     /* 0 none, 1 sigmoid, 2 tanh */
} narde_value_mlp;

/* narde_afterstates with value f32[cap] in place of feat and obs: the same
 * rows in the same order, offsets, cap rule and optional arrays (the count
 * pass and the scan are that call's).  value[r] = v(row r) for a row of
 * reward 0; a terminal row's is its outcome: reward as a float, negated when
 * perspective is 1 (white's values) and the side that made the move is
 * black; perspective 0: the mover's values (narde_afterstate_pick's two).
 * Nothing at or past cap is touched.  Stream-ordered, allocates nothing, no
 * synchronise, graph-capturable.  NARDE_EINVAL before any device call: NULL
 * net, value or weights, hidden outside 1..NARDE_VALUE_HIDDEN_MAX, ld_w1t <
 * hidden (or above 2^20), an unknown activation or perspective, a negative
 * cap. */
int narde_afterstates_scored(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                             int32_t *row_env, int16_t *codes, int8_t *reward,
                             const narde_value_mlp *net, int perspective, float *value, void *stream);

/* Two-ply lookahead over narde_afterstates_scored's rows (REF2; DESIGN.md
 * section 17).  The rows, their order, offsets, row_env, codes, reward, the
 * cap rule and dice == NULL are exactly that call's.  value[r] is WHITE's
 * value of row r:
 *   a terminal row (reward != 0): its outcome, as the scored call gives it;
 *   any other row: the mean, over the opponent's ordered rolls (a, b) in the
 *   env's dice mode (36 pairs for NARDE_DICE_ALL36, the 30 unequal ones for
 *   NARDE_DICE_NODOUBLES, equal weight each), of the best reply m(r, a, b).
 * Let s_r be the position row r leaves: its record after the step, the
 * mover flipped, the first-turn flags as narde_step leaves them.  If s_r
 * with the roll (a, b) has rows in narde_afterstates' sense, m is the
 * smallest of their narde_afterstates_scored values (perspective 1) when
 * the side to reply is black, the largest when it is white; terminal
 * replies enter with their outcome.  If it has none, m is the value (a
 * terminal one: the outcome) of the position narde_step(actions = (0, 0),
 * that roll, autoreset = 0) leaves.  That is s_r with the mover flipped --
 * a pass -- with one exception, which the step's own result defines: code 0
 * is the bear-off from point 0, so where that move is legal and every play
 * that starts with it needs a second move no code can express, the step
 * bears the checker off (and a second one from point 0 if the other die
 * allows) although no row says so (4 of the 7,732 no-reply (row, roll)
 * pairs of tests/test_lookahead_cpu.py).  The TimeLimit is not looked at.
 * The rolls are evaluated as the 36 (30) ordered pairs: (a, b) and (b, a)
 * can leave different afterstates (narde_env.py:63-83 drops the first die
 * in roll order when a bear-off's distance is not rolled).
 * perspective must be 1: the mover's values have no successor sign under a
 * bounded output (narde_value_td_apply's reason).
 * The same inputs give the same bits on every call, whatever cap: no float
 * atomics, a row's per-roll values are summed by one lane in the order a
 * outer, b inner, in double, the mean rounded to float once.
 * scratch: device memory, 16-B aligned, scratch_bytes >=
 * NARDE_LOOKAHEAD_SCRATCH_BYTES(cap): the rows' 32-byte records, kept
 * between the call's passes; its contents afterwards are unspecified.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable: the
 * lookahead pass is launched over cap rows (never more than the rows B envs
 * can have) and its waves leave at or past min(offsets[B], cap); nothing at
 * or past cap is touched.  NARDE_EINVAL before any device call:
 * narde_afterstates_scored's cases, perspective != 1, a NULL, too small or
 * misaligned scratch. */
#define NARDE_LOOKAHEAD_SCRATCH_BYTES(cap) (32 * (int64_t)(cap))
int narde_afterstates_lookahead(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                                int32_t *row_env, int16_t *codes, int8_t *reward,
                                const narde_value_mlp *net, int perspective, float *value,
                                void *scratch, int64_t scratch_bytes, void *stream);

/* Whole value-greedy games in one launch, one net per colour (REF2; DESIGN.md
 * section 19).  For k = 0 .. plies - 1 every env e does what these three
 * calls do:
 *   narde_afterstates_scored(dice = NULL, the net of e's mover, perspective 1);
 *   narde_afterstate_pick(perspective 1, epsilon, seed, tag = *tag + k) -- the
 *     same tie rule (the lowest row), NaN rule (the first NaN) and explore
 *     draw Philox4x32-10({*tag + k, e, 0, 5}, seed); epsilon NULL: greedy;
 *   narde_step(those actions, dice = NULL, autoreset = 1).
 * An env with no row steps with (0, 0) -- a pass, with
 * narde_afterstates_lookahead's one exception (the bear-off from point 0).
 * The mover's net is net_black when black moves, net_white otherwise; they
 * may be the same struct.  A NULL net makes that colour's plies the
 * random-legal policy's: bit for bit narde_step(actions = NULL, dice = NULL,
 * autoreset = 1), drawn from the same words of the ply stream.  Both NULL is
 * NARDE_EINVAL (that is narde_selfplay).
 * Outputs, each optional, laid out [plies][B]: dice u8[2] the roll used,
 * actions i16[2] the codes played, value f32 white's value of the picked row
 * (a terminal row's: its outcome; NaN on a random ply and on a ply with no
 * row), reward / terminated / truncated as narde_step gives them.  The
 * statistics accumulate as in narde_step and t advances by plies.  No row,
 * feature or per-row value goes to memory; the same inputs give the same bits.
 * The handle has no rule set of its own: the plies are REF2's (on a
 * rules = "full4" env the Python calls raise).
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable (one
 * kernel node; epsilon and tag are read on the device).  NARDE_EINVAL before
 * any device call: a NULL handle, narde_afterstates_scored's net errors for
 * either net, plies < 1, epsilon and tag not both set or both NULL, actions
 * not 4-B aligned. */
int narde_value_rollout(narde_env *env, int plies, const narde_value_mlp *net_white,
                        const narde_value_mlp *net_black, const float *epsilon, uint64_t seed,
                        const int64_t *tag, uint8_t *dice, int16_t *actions, float *value,
                        int32_t *reward, uint8_t *terminated, uint8_t *truncated, void *stream);

/* narde_value_rollout with one more optional output:
 * records u32[plies][B][8], 16-B aligned -- records[k][e] is env e's 32-byte
 * record (its two planes, p0 then p1) as ply k found it: after ply k - 1's
 * step and auto-reset, before ply k's roll is applied.  It is what
 * narde_value_td_window trains on.  records == NULL is narde_value_rollout
 * itself, bit for bit; every other output and the final state do not depend
 * on records.  NARDE_EINVAL: narde_value_rollout's cases, records not 16-B
 * aligned. */
int narde_value_rollout_records(narde_env *env, int plies, const narde_value_mlp *net_white,
                                const narde_value_mlp *net_black, const float *epsilon, uint64_t seed,
                                const int64_t *tag, uint8_t *dice, int16_t *actions, float *value,
                                int32_t *reward, uint8_t *terminated, uint8_t *truncated,
                                void *records, void *stream);

/* narde_afterstates_scored over narde_turn_afterstates' rows (FULL4), the overflow path
 * included; that call's workspace rule holds (the handle's first call of
 * either, outside capture). */
int narde_turn_afterstates_scored(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                                  int32_t *row_env, int8_t *play, int8_t *reward,
                                  const narde_value_mlp *net, int perspective, float *value,
                                  void *stream);

/* Two-ply lookahead over narde_turn_afterstates_scored's rows (FULL4;
 * DESIGN.md section 18).  The rows, their order, offsets, row_env, play,
 * reward, the cap rule, dice == NULL and the workspace rule are exactly that
 * call's.  value[r] is WHITE's value of row r:
 *   a terminal row (reward != 0): its outcome, as the scored call gives it;
 *   any other row: sum w m(r, roll) / sum w over the opponent's rolls.
 * Let s_r be the position row r's play leaves under narde_step_full(play,
 * dice, autoreset = 0): the mover flipped and both first-turn flags as that
 * step leaves them (the side that moved has its flag cleared; the replier's
 * decides the reply's head limit on 3-3, 4-4 and 6-6).  For a roll, the reply
 * set is s_r's rows in narde_turn_afterstates' sense -- whole turns, the
 * max-dice-used rule, two different dice with only one playable taking the
 * higher die's nodes if it has any --, exact for every position (levels of up
 * to NARDE_TURN_AFT_MAX nodes).  m is the smallest of the replies'
 * narde_turn_afterstates_scored values (perspective 1) when the side to reply
 * is black, the largest when it is white; terminal replies enter with their
 * outcome.  A roll with no legal sub-move (a pass) takes the value of the
 * position narde_step_full with an all -1 play leaves: always s_r with the
 * mover flipped and nothing else changed -- FULL4 has no analogue of REF2's
 * code-0 exception (all 784 pass (row, roll) pairs of
 * tests/test_turn_lookahead_cpu.py).  The TimeLimit is not looked at.
 * The dice of a roll are ordered before the turn is enumerated, so (a, b)
 * and (b, a) give the same rows in the same order (checked against the
 * oracle on that test's whole input set): the unordered rolls a <= b are
 * evaluated, a outer ascending, b inner ascending, w = 1 for a double and 2
 * otherwise (36 in all); under NARDE_DICE_NODOUBLES the 15 unequal rolls,
 * equal weight each.
 * perspective must be 1 (narde_afterstates_lookahead's reason).
 * The same inputs give the same bits on every call, whatever cap and however
 * the work is split over waves: no float atomics, every (row, roll) best is
 * written by one wave to a slot of its own, and one thread sums a row's
 * slots in that roll order in double and rounds the mean to float once.
 * scratch: device memory, 16-B aligned, scratch_bytes >=
 * NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES(cap): 128 B a row (its 32-byte record,
 * the rolls' bests, the rolls to redo with a larger frontier); its contents
 * afterwards are unspecified.  Stream-ordered, allocates nothing, no
 * synchronise, graph-capturable once the handle's workspace exists; nothing at
 * or past cap is touched.  NARDE_EINVAL before any device call:
 * narde_turn_afterstates_scored's cases, perspective != 1, a NULL, too small
 * or misaligned scratch. */
#define NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES(cap) (128 * (int64_t)(cap))
int narde_turn_afterstates_lookahead(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                                     int32_t *row_env, int8_t *play, int8_t *reward,
                                     const narde_value_mlp *net, int perspective, float *value,
                                     void *scratch, int64_t scratch_bytes, void *stream);

/* Whole value-greedy FULL4 games in one launch, one net per colour (DESIGN.md
 * section 20): narde_value_rollout under FULL4's whole turns.  For k = 0 ..
 * plies - 1 every env e does what these three calls do:
 *   narde_turn_afterstates_scored(dice = NULL, the net of e's mover,
 *     perspective 1);
 *   narde_turn_pick(perspective 1, epsilon, seed, tag = *tag + k) -- the same
 *     tie rule (the lowest row), NaN rule (the first NaN) and explore draw
 *     Philox4x32-10({*tag + k, e, 0, 5}, seed), the explored row of ordinal
 *     mulhi(r1, count); epsilon NULL: greedy;
 *   narde_step_full(that play, dice = NULL, autoreset = 1).
 * An env with no row steps with the all -1 play: a pass (FULL4 has no
 * analogue of REF2's code-0 exception).  The mover's net is net_black when
 * black moves, net_white otherwise; they may be the same struct.  A NULL net
 * makes that colour's plies the random-legal policy's: bit for bit
 * narde_step_full(play = NULL, dice = NULL, autoreset = 1), drawn from the
 * same words of the ply stream.  Both NULL is NARDE_EINVAL (that is
 * narde_selfplay).
 * Outputs, each optional, laid out [plies][B]: dice u8[2] the roll used, play
 * i8[4][2] the (from, die) sub-moves played, -1 padding -- a net's ply: exactly
 * what narde_step_full would be given; a random ply: what it played --, 8-B
 * aligned; value f32 white's value of the row played (a terminal row's: its
 * outcome; NaN on a random ply and on a pass); reward / terminated / truncated
 * as narde_step_full gives them.  The statistics accumulate as in
 * narde_step_full and t advances by plies.  No row, feature or per-row value
 * goes to memory.
 * scratch: device memory, 16-B aligned, cut into pieces of
 * NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1) bytes, one a wave: the launch is
 * min(B, scratch_bytes / that) one-wave workgroups, wave w playing envs w,
 * w + waves, ..., each for all its plies (a static assignment: nothing spins,
 * nothing is claimed with an atomic).  A wave walks a turn's levels with 256
 * nodes a level on chip and, when a level outgrows that, again in its piece
 * (NARDE_TURN_AFT_MAX nodes a level): exact for every position.  The same
 * inputs give the same bits whatever scratch_bytes; the contents of scratch
 * afterwards are unspecified.  narde_turn_value_rollout_waves gives the number
 * of waves the device keeps resident for the kernel (launches nothing): more
 * pieces than that buy nothing.  The handle's narde_turn_afterstates workspace
 * is not needed.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable (one
 * kernel node; epsilon and tag are read on the device).  NARDE_EINVAL before
 * any device call: a NULL handle, narde_value_rollout's cases for either net,
 * plies < 1, epsilon and tag not both set or both NULL, play not 8-B aligned,
 * a NULL or misaligned scratch, scratch_bytes below one piece. */
#define NARDE_TURN_ROLLOUT_SCRATCH_BYTES(waves) (83536 * (int64_t)(waves))
int narde_turn_value_rollout_waves(const narde_env *env, int *waves);
int narde_turn_value_rollout(narde_env *env, int plies, const narde_value_mlp *net_white,
                             const narde_value_mlp *net_black, const float *epsilon, uint64_t seed,
                             const int64_t *tag, uint8_t *dice, int8_t *play, float *value,
                             int32_t *reward, uint8_t *terminated, uint8_t *truncated,
                             void *scratch, int64_t scratch_bytes, void *stream);

/* narde_turn_value_rollout with narde_value_rollout_records' optional output
 * (the same layout and the same moment of a ply).  NARDE_EINVAL:
 * narde_turn_value_rollout's cases, records not 16-B aligned. */
int narde_turn_value_rollout_records(narde_env *env, int plies, const narde_value_mlp *net_white,
                                     const narde_value_mlp *net_black, const float *epsilon,
                                     uint64_t seed, const int64_t *tag, uint8_t *dice, int8_t *play,
                                     float *value, int32_t *reward, uint8_t *terminated,
                                     uint8_t *truncated, void *scratch, int64_t scratch_bytes,
                                     void *records, void *stream);

/* Round-robin leagues in one launch: a value net per env and colour
 * (DESIGN.md section 27).  The two records rollouts above with the nets taken,
 * per env, from a table in device memory instead of from two arguments.
 *
 * narde_net_table writes the kernels' view of n_nets nets (a host array of
 * narde_value_mlp) into table: device memory, 16-B aligned, table_bytes >=
 * NARDE_LEAGUE_TABLE_BYTES(n_nets).  An entry is opaque and 64 B (the
 * kernels' view of a net is 56 B).  The nets travel by value in the arguments
 * of small kernel launches on the stream (16 nets a launch): no host copy, so
 * the call is stream-ordered, allocates nothing, does not synchronise and is
 * graph-capturable.  The weights are not copied -- an entry holds the net's
 * pointers --, so weights changed between two launches are seen by the second,
 * as with every other call; the nets array itself is not needed after the call
 * returns.  Needs no handle.  NARDE_EINVAL before any device call: a negative
 * device, NULL nets or table, n_nets outside 1..NARDE_LEAGUE_NETS_MAX, table
 * misaligned, table_bytes too small, any net's error (narde_value_rollout's
 * cases; the message names the net's index). */
#define NARDE_LEAGUE_NETS_MAX 64
#define NARDE_LEAGUE_TABLE_BYTES(n) (64 * (int64_t)(n))
int narde_net_table(int device, int n_nets, const narde_value_mlp *nets /* host array */,
                    void *table /* device, 16-B aligned */, int64_t table_bytes, void *stream);

/* narde_value_rollout_records (REF2) except for where the nets come from: env
 * e's white plies are played under net white[e] of the table and its black
 * plies under net black[e], for every game the env plays inside the launch
 * (the assignment survives auto-resets).  white, black: device i32[B], 4-B
 * aligned, read on the device.  An index outside 0 .. n_nets - 1 (-1, n_nets,
 * INT32_MIN, ...) makes that colour of that env play the random-legal policy,
 * bit for bit narde_step(actions = NULL, dice = NULL, autoreset = 1), drawn
 * from the same words of the ply stream; no table entry is read for it.  Both
 * colours random in one env is allowed (that env plays narde_selfplay's
 * plies), and so is white[e] == black[e] (self-play of one net).
 * Env e's outputs, final record and statistics are, bit for bit, what
 * narde_value_rollout_records gives env e of a handle in the same state under
 * (nets[white[e]], nets[black[e]]) with the same epsilon, seed and tag.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable (one
 * kernel node: white, black, epsilon, tag and the table are read on the
 * device).  No row or per-row value goes to memory.
 * A table not written by narde_net_table for at least n_nets nets is the
 * caller's error, as a bad weight pointer is: it is not detected.
 * NARDE_EINVAL before any device call: a NULL handle, plies < 1, NULL table,
 * white or black, table not 16-B aligned, white or black not 4-B aligned,
 * n_nets outside 1..NARDE_LEAGUE_NETS_MAX, epsilon and tag not both set or
 * both NULL, actions not 4-B aligned, records not 16-B aligned. */
int narde_value_rollout_league(narde_env *env, int plies, const void *table, int n_nets,
                               const int32_t *white, const int32_t *black, /* device i32[B] */
                               const float *epsilon, uint64_t seed, const int64_t *tag,
                               uint8_t *dice, int16_t *actions, float *value, int32_t *reward,
                               uint8_t *terminated, uint8_t *truncated, void *records, void *stream);

/* The same over narde_turn_value_rollout_records (FULL4): play i8[4][2] 8-B
 * aligned, scratch and scratch_bytes with that call's piece rule.  A wave
 * plays envs w, w + waves, ... one after another and takes each env's pair
 * when it starts that env; the same inputs give the same bits whatever
 * scratch_bytes.  NARDE_EINVAL: narde_value_rollout_league's cases with play
 * not 8-B aligned in place of actions, a NULL or misaligned scratch,
 * scratch_bytes below one piece. */
int narde_turn_value_rollout_league(narde_env *env, int plies, const void *table, int n_nets,
                                    const int32_t *white, const int32_t *black,
                                    const float *epsilon, uint64_t seed, const int64_t *tag,
                                    uint8_t *dice, int8_t *play, float *value, int32_t *reward,
                                    uint8_t *terminated, uint8_t *truncated, void *scratch,
                                    int64_t scratch_bytes, void *records, void *stream);

/* Monte-Carlo playouts: given positions played to the end under value nets
 * (DESIGN.md section 22).
 *
 * narde_state_records packs n positions (narde_set_state's arrays, device
 * memory) into the 32-B records the records rollouts write: records u32[n][8],
 * planes p0 then p1, 16-B aligned, the ply counter t, elapsed 0.  Stateless,
 * no validation on the device.  NARDE_EINVAL: a NULL array, n < 1, n >= 2^31,
 * records misaligned.
 *
 * narde_value_playout (REF2): roots u32[n][8] records (a records rollout's
 * output as it stands).  Trial j of root i, local index q = i * trials + j,
 * plays from roots[i] -- with its t -- exactly the plies narde_value_rollout
 * (epsilon NULL) plays for an env with that record at env index q of a handle
 * made with seed, env_id_offset = id_base, the calling handle's dice mode and
 * max_episode_steps = 0: the same ply stream, expansion, tie and NaN rules,
 * mover's net, random-legal policy for a NULL net (both NULL: NARDE_EINVAL),
 * and code-0 exception.  The trial stops after the first ply that terminates,
 * or after max_plies plies; nothing is reset and no TimeLimit is looked at.
 * NARDE_PLAYOUT_COMMON_DICE: trial j's env index and id are j and id_base + j
 * for every root (common random numbers).  Of the handle only the device and
 * the dice mode are read; nothing of it is written.
 * Outputs: sums i32[n][4] (required; zeroed by the call) = finished trials,
 * the sum of white's outcomes (the terminating ply's reward, negated when
 * black made it), the sum of their squares, the plies played by all trials;
 * optional outcome i8[n][trials] (0: unfinished), length i32[n][trials], leaf
 * f32[n][trials]: for an unfinished trial white's value of the record it
 * stopped at, as narde_value_td_trace's v, under that record's mover's net
 * (the other colour's if it has none); NaN for a finished trial.  The sums are
 * integer adds: the same bits for any launch geometry.
 * A root in which a side has 15 checkers off already is not a position of a
 * game: its numbers are unspecified.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable (two
 * kernel nodes: the sums' zeros, the trials).  NARDE_EINVAL before any device call: a NULL
 * handle, roots or sums; narde_value_rollout's cases for either net; both nets
 * NULL; n, trials or max_plies < 1; n * trials >= 2^31; trials * max_plies >=
 * 2^31; an unknown flag; roots not 16-B aligned; id_base < 0 or id_base + n *
 * trials >= 2^32.
 *
 * narde_turn_value_playout (FULL4): the same over narde_turn_value_rollout's
 * whole turns, a pass when there is no row.  scratch as there: pieces of
 * NARDE_TURN_ROLLOUT_SCRATCH_BYTES(1), trial q played by wave q mod waves;
 * the same bits whatever scratch_bytes.  NARDE_EINVAL also: a NULL or
 * misaligned scratch, scratch_bytes below one piece. */
int narde_state_records(int device, int64_t n, const int8_t *board, const uint8_t *off,
                        const uint8_t *first_turn, const int8_t *player, uint32_t t,
                        void *records, void *stream);
#define NARDE_PLAYOUT_COMMON_DICE 1
int narde_value_playout(narde_env *env, int64_t n, const void *roots, int trials, int max_plies,
                        const narde_value_mlp *net_white, const narde_value_mlp *net_black,
                        uint64_t seed, int64_t id_base, int flags, int32_t *sums, int8_t *outcome,
                        int32_t *length, float *leaf, void *stream);
int narde_turn_value_playout(narde_env *env, int64_t n, const void *roots, int trials, int max_plies,
                             const narde_value_mlp *net_white, const narde_value_mlp *net_black,
                             uint64_t seed, int64_t id_base, int flags, int32_t *sums,
                             int8_t *outcome, int32_t *length, float *leaf, void *scratch,
                             int64_t scratch_bytes, void *stream);

/* Playout-greedy play: a roll's rows with their records, each env's K best
 * rows as playout roots, and the pick over the playouts' sums (DESIGN.md
 * section 23).  The chain -- records, top-K, narde_value_playout, pick,
 * narde_step -- has static shapes and is graph-capturable.
 *
 * narde_afterstates_records / narde_turn_afterstates_records:
 * narde_afterstates_scored / narde_turn_afterstates_scored with one more
 * output; the rows, their order, offsets, the cap rule, dice == NULL and the
 * FULL4 workspace rule (the handle's first call outside capture; the overflow
 * tiers included) are the same, and one expansion is paid.  records
 * u32[cap][8], 16-B aligned: records[r] is the record narde_step(codes[r],
 * dice, autoreset = 0) -- FULL4: narde_step_full(play[r], dice, autoreset = 0)
 * -- leaves in env row_env[r], in the layout the records rollouts write (p0
 * then p1): the mover flipped unless the row is terminal, the first-turn flags
 * and elapsed as that step leaves them, word 7 the env's ply counter as the
 * step leaves it.  Nothing at or past cap is touched.  net == NULL with value
 * == NULL: the records alone.  NARDE_EINVAL before any device call: the scored
 * call's cases; records NULL (that is the scored call) or not 16-B aligned;
 * net and value not both set or both NULL.
 *
 * narde_rows_topk (both rule sets: it works on offsets): sel i32[B][k], slots
 * 0 .. m - 1 with m = min(k, env e's rows below cap) = the env's best rows,
 * best first, under exactly the picks' order (epsilon NULL): perspective 0 the
 * largest value[r * ld_value], perspective 1 the largest when white moves (the
 * env's record) and the smallest when black does, the lowest row on ties, NaNs
 * first in row order; slots m .. k - 1 are -1.  sel[e][0] is the row
 * narde_afterstate_pick / narde_turn_pick return.  With records (the call
 * above's) roots u32[B][k][8] gets roots[e][i] = records[sel[e][i]], an empty
 * slot the none record: seven zero words and word 6 = NARDE_RECORD_NONE_WORD6
 * (an empty board, both sides' 15 checkers off).  A wave an env, no atomics,
 * the same bits on every call.  NARDE_EINVAL: a NULL handle, offsets, value or
 * sel; k outside 1 .. NARDE_TOPK_MAX; an unknown perspective; cap < 0;
 * ld_value < 1; roots and records not both set or both NULL, either not 16-B
 * aligned; B * k >= 2^31.
 *
 * narde_playout_pick / narde_turn_playout_pick: per env the slot to play among
 * its k candidates, from a playout call over the B * k roots (slot i of env e:
 * row r = sel[e][i], sums row e * k + i, leaf row e * k + i).  The values are
 * white's (value from a perspective-1 call).  A slot's score: r < 0 -- no
 * candidate (score: NaN); reward[r] != 0 -- value[r], the known outcome; leaf
 * NULL -- (float)((double)points / finished), or value[r] when no trial
 * finished; leaf given -- (float)(((double)points + S) / trials), S the slot's
 * non-NaN leaves added in trial order in double.  The largest score when white
 * moves, the smallest when black does, the lowest slot on ties, NaN as the
 * picks take it.  actions i16[B][2] / out_play i8[B][4][2] are ready for
 * narde_step / narde_step_full: (0, 0) or the all -1 play, and row -1, for an
 * env with no candidate.  Optional row i32[B], score f32[B][k].  Integer sums
 * and one rounding: the same bits on every call.  NARDE_EINVAL: a NULL handle,
 * sel, value, reward, sums, codes / play or actions / out_play; k outside
 * 1 .. NARDE_TOPK_MAX; trials < 1; cap < 0; ld_value < 1; B * k * trials >=
 * 2^31; codes and actions not 4-B (play and out_play not 8-B) aligned.
 *
 * All stream-ordered, allocate nothing, no synchronise. */
#define NARDE_TOPK_MAX 64
#define NARDE_RECORD_NONE_WORD6 0xFFu
int narde_afterstates_records(narde_env *env, const uint8_t *dice, int64_t cap, int32_t *offsets,
                              int32_t *row_env, int16_t *codes, int8_t *reward,
                              const narde_value_mlp *net, int perspective, float *value,
                              void *records, void *stream);
int narde_turn_afterstates_records(narde_env *env, const uint8_t *dice, int64_t cap,
                                   int32_t *offsets, int32_t *row_env, int8_t *play, int8_t *reward,
                                   const narde_value_mlp *net, int perspective, float *value,
                                   void *records, void *stream);
int narde_rows_topk(narde_env *env, const int32_t *offsets, int64_t cap, const float *value,
                    int64_t ld_value, int perspective, int k, const void *records, int32_t *sel,
                    void *roots, void *stream);
int narde_playout_pick(narde_env *env, int k, const int32_t *sel, int64_t cap, const float *value,
                       int64_t ld_value, const int8_t *reward, const int16_t *codes, int trials,
                       const int32_t *sums, const float *leaf, int16_t *actions, int32_t *row,
                       float *score, void *stream);
int narde_turn_playout_pick(narde_env *env, int k, const int32_t *sel, int64_t cap,
                            const float *value, int64_t ld_value, const int8_t *reward,
                            const int8_t *play, int trials, const int32_t *sums, const float *leaf,
                            int8_t *out_play, int32_t *row, float *score, void *stream);

/* Two-ply values of given positions, and the pick over given slot scores
 * (DESIGN.md section 25): what narde_afterstates_lookahead /
 * narde_turn_afterstates_lookahead compute a row, for any records -- a
 * narde_rows_topk's roots (pruned two-ply play), a rollout window's recorded
 * positions (two-ply training targets), narde_state_records' positions.
 *
 * narde_records_lookahead (REF2), narde_turn_records_lookahead (FULL4):
 * records u32[n][8], 16-B aligned, in the public record layout (what
 * narde_state_records, the records rollouts, narde_*_afterstates_records and
 * narde_rows_topk's roots write), are only read.  value[i] is WHITE's value of
 * records[i] with its mover about to roll: exactly the per-row definition of
 * the two calls above with s_r := records[i] -- REF2 the mean over the 36 (30
 * under NARDE_DICE_NODOUBLES) ordered rolls of the mover's best
 * narde_afterstates_scored value at perspective 1 (black the smallest, white
 * the largest; terminal replies at their outcome; a roll with no reply what
 * narde_step((0, 0)) leaves, the code-0 exception included); FULL4 the
 * weighted mean over the 21 (15) unordered rolls of the best whole-turn
 * reply, exact through both overflow tiers, a pass scoring the record with
 * the mover flipped.  The summation order and the one rounding are those
 * calls': on the records of a roll's rows the values are theirs bit for bit.
 * Word 7 -- the ply counter, not a reward -- and elapsed are ignored.  A
 * record in which either side has 15 checkers off (a finished game;
 * narde_rows_topk's none record) gets value[i] = NaN.  Of the handle only the
 * device, the dice mode and (FULL4) the overflow workspace are read; no env is
 * touched.  The same bits on every call and for either launch shape (up to
 * 3,072 records a record's rolls go over four waves, past that one wave a
 * record).  Nothing at or past value[n] is written.
 * scratch (FULL4): device memory, 16-B aligned, scratch_bytes >=
 * NARDE_TURN_LOOKAHEAD_SCRATCH_BYTES(n): a pack pass copies each record into
 * its 128-B row piece; its contents afterwards are unspecified.
 * Stream-ordered, allocate nothing, no synchronise, graph-capturable -- FULL4
 * once the handle's workspace exists (narde_turn_afterstates' rule: the
 * handle's first FULL4 call, this one included, outside capture).
 * NARDE_EINVAL before any device call: a NULL handle, records, net or value;
 * n < 1 or n >= 2^31; records not 16-B aligned; the scored call's net cases;
 * FULL4: a NULL, misaligned or too small scratch.
 *
 * narde_slot_pick / narde_turn_slot_pick: narde_playout_pick /
 * narde_turn_playout_pick with a given score a slot in place of the playouts'
 * sums.  slot_score f32[B][k]; a slot's score: sel < 0 -- NaN (no candidate,
 * never picked); reward[r] != 0 -- value[r * ld_value], the known outcome;
 * else slot_score[e][i].  The largest score when white moves (the env's
 * record), the smallest when black does, the lowest slot on ties, NaN as the
 * picks take it.  The outputs are that call's: actions / out_play ready for
 * narde_step / narde_step_full, (0, 0) or the all -1 play and row -1 for an
 * env with no candidate; optional row i32[B], score f32[B][k] (score may be
 * slot_score itself).  NARDE_EINVAL: a NULL handle, sel, value, reward,
 * slot_score, codes / play or actions / out_play; k outside 1 ..
 * NARDE_TOPK_MAX; cap < 0; ld_value < 1; B * k >= 2^31; codes and actions not
 * 4-B (play and out_play not 8-B) aligned. */
int narde_records_lookahead(narde_env *env, int64_t n, const void *records,
                            const narde_value_mlp *net, float *value, void *stream);
int narde_turn_records_lookahead(narde_env *env, int64_t n, const void *records,
                                 const narde_value_mlp *net, float *value, void *scratch,
                                 int64_t scratch_bytes, void *stream);
int narde_slot_pick(narde_env *env, int k, const int32_t *sel, int64_t cap, const float *value,
                    int64_t ld_value, const int8_t *reward, const int16_t *codes,
                    const float *slot_score, int16_t *actions, int32_t *row, float *score,
                    void *stream);
int narde_turn_slot_pick(narde_env *env, int k, const int32_t *sel, int64_t cap, const float *value,
                         int64_t ld_value, const int8_t *reward, const int8_t *play,
                         const float *slot_score, int8_t *out_play, int32_t *row, float *score,
                         void *stream);

/* TD(lambda) on that value MLP, trained in place on the device (DESIGN.md
 * section 16). narde_value_mlp_train: narde_value_mlp's fields, the weights
 * writable, and an optional mirror of the first layer: w1, row-major
 * [hidden][ld_w1] (ld_w1 >= 198), w1[h * ld_w1 + c] = w1t[c * ld_w1t + h] --
 * a torch Linear(198, hidden).weight; NULL: none.  Every update writes w1t
 * and the mirror the same bits, so the scored calls above see the new
 * weights at their next launch.
 *
 * A trace row is P = 200 * hidden + 1 floats: T[c * hidden + h] = the trace
 * of W1[h][c] for column c < 198 (dense, whatever ld_w1t), then b1's at
 * 198 * hidden, w2's at 199 * hidden, b2's at 200 * hidden.  trace
 * f32[B][ld_trace], 16-B aligned, ld_trace >= P and a multiple of 4; floats
 * past P of a row are never touched. */
typedef struct narde_value_mlp_train {
  float *w1t;          /* f32[198][ld_w1t] */
  int64_t ld_w1t;      /* >= hidden */
  float *b1;           /* f32[hidden] */
  float *w2;           /* f32[hidden] */
  float *b2;           /* f32[1] */
  int32_t hidden;      /* 1 .. NARDE_VALUE_HIDDEN_MAX */
  int32_t hidden_act;  /* 0 sigmoid, 1 tanh, 2 relu */
  int32_t out_act;     /* 0 none, 1 sigmoid, 2 tanh */
  float *w1;           /* f32[hidden][ld_w1] or NULL */
  int64_t ld_w1;       /* >= 198 when w1 is given */
} narde_value_mlp_train;

/* For every env e, from its record as it stands: v[e] = v(s_e) (white's
 * value, the net's forward), black[e] (u8) = 1 when black is to move, and
 *   trace[e] = decay * trace[e] + grad_theta v(s_e).
 * decay == 0 overwrites the row without reading it (uninitialised memory is
 * fine).  Stream-ordered, allocates nothing, no synchronise,
 * graph-capturable.  NARDE_EINVAL before any device call: a NULL env, net,
 * trace, v, black or weight array, hidden outside
 * 1..NARDE_VALUE_HIDDEN_MAX, ld_w1t < hidden (or above 2^20), ld_w1 < 198
 * with a mirror, an unknown activation, ld_trace < P or not a multiple of
 * 4, trace not 16-B aligned. */
int narde_value_td_trace(narde_env *env, const narde_value_mlp_train *net, float decay, float *trace,
                         int64_t ld_trace, float *v, uint8_t *black, void *stream);

/* The update after the step that followed narde_value_td_trace; v and black
 * are that call's, reward i32[B], terminated and truncated u8[B] the
 * step's.  Per env
 *   target = the outcome -- reward, negated when black[e] -- if terminated,
 *            v[e] if truncated (delta 0: under autoreset the successor is
 *            gone), else gamma * v(s'_e) from the env's record as it stands,
 *            under the weights before this update;
 *   delta_e = target - v[e], written to delta f32[B] if not NULL;
 * then theta += alpha * sum_e delta_e * trace[e] into w1t, b1, w2, b2 and
 * the mirror, and the trace rows of terminated or truncated envs are zeroed.
 * The sum has one order -- partial rows over slabs of NARDE_TD_SLAB envs in
 * env order, kept in scratch, then the partial rows in slab order -- and no
 * float atomics: the same inputs give the same bits.  scratch: device
 * memory, 16-B aligned, scratch_floats >= NARDE_TD_SCRATCH_FLOATS(B, hidden).
 * perspective must be 1 (white's values): the mover's have no successor
 * sign under a bounded output.  Stream-ordered, allocates nothing, no
 * synchronise, graph-capturable.  NARDE_EINVAL before any device call:
 * narde_value_td_trace's cases, a NULL reward, terminated, truncated or
 * scratch, perspective != 1, scratch too small or misaligned. */
#define NARDE_TD_SLAB 64
#define NARDE_TD_SCRATCH_FLOATS(B, hidden) \
  ((((int64_t)(B) + 3) / 4) * 4 + (((int64_t)(B) + NARDE_TD_SLAB - 1) / NARDE_TD_SLAB) * (200 * (int64_t)(hidden) + 4))
int narde_value_td_apply(narde_env *env, const narde_value_mlp_train *net, float *trace, int64_t ld_trace,
                         const float *v, const uint8_t *black, const int32_t *reward,
                         const uint8_t *terminated, const uint8_t *truncated, float alpha, float gamma,
                         int perspective, float *scratch, int64_t scratch_floats, float *delta,
                         void *stream);

/* Windowed (truncated) TD(lambda): one weight update from a recorded window
 * of K = plies plies.  records u32[K][B][8], reward
 * i32[K][B], terminated and truncated u8[K][B] are laid out as the records
 * rollouts above write them; the call does not care how they were produced.
 * Under the weights as they are on entry, per env e:
 *   s_k = records[k][e] for k < K, s_K = the env's record as it stands;
 *   v_k = v(s_k), white's value, k = 0 .. K; black_k = s_k's mover bit;
 *   target_k = the outcome -- reward[k], negated when black_k -- if
 *              terminated[k], v_k if truncated[k], else gamma * v_{k+1};
 *   delta_k = target_k - v_k, written to delta f32[K][B] if not NULL;
 *   G_K = 0, G_k = delta_k + c_k * G_{k+1}, c_k = 0 where ply k ended an
 *         episode (terminated or truncated), gamma * lam elsewhere;
 * then theta += alpha * sum_e sum_k G_k * grad_theta v(s_k) into w1t, b1, w2,
 * b2 and the mirror, the same bits to both.  With the weights fixed over the
 * window this equals the backward view's sum_k delta_k trace_k; states before
 * the window get nothing from its errors (no credit crosses the left edge).
 * No trace array exists: a sample's gradient goes from its record's own
 * columns straight into an accumulator on chip.  The sum has one order and no
 * float atomics -- the samples in k * B + e order in slabs of
 * NARDE_TD_WINDOW_SLAB, every element of a slab's partial row taking its
 * addends in sample order, then the partial rows in slab order --: the same
 * inputs give the same bits.
 * scratch: device memory, 16-B aligned, scratch_floats >=
 * NARDE_TD_WINDOW_SCRATCH_FLOATS(B, plies, hidden).  On return it holds
 * v f32[K + 1][B] at its start and G f32[K][B] behind it, (K + 1) * B rounded
 * up to a multiple of 4 floats in; the rest is unspecified.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable once
 * the device has seen one call (the first announces the gradient kernel's
 * LDS).  NARDE_EINVAL before any device call: narde_value_td_trace's net
 * cases, a NULL env, records, reward, terminated, truncated or scratch,
 * plies < 1, (plies + 1) * B at or above 2^31, lam outside [0, 1], records or
 * scratch not 16-B aligned, scratch too small. */
#define NARDE_TD_WINDOW_SLAB 128
#define NARDE_TD_WINDOW_SCRATCH_FLOATS(B, plies, hidden)                                          \
  (((((int64_t)(plies) + 1) * (int64_t)(B) + 3) / 4) * 4 +                                        \
   (((int64_t)(plies) * (int64_t)(B) + 3) / 4) * 4 +                                              \
   (((int64_t)(plies) * (int64_t)(B) + NARDE_TD_WINDOW_SLAB - 1) / NARDE_TD_WINDOW_SLAB) *        \
       (200 * (int64_t)(hidden) + 4))
int narde_value_td_window(narde_env *env, const narde_value_mlp_train *net, int plies,
                          const void *records, const int32_t *reward, const uint8_t *terminated,
                          const uint8_t *truncated, float alpha, float lam, float gamma,
                          float *scratch, int64_t scratch_floats, float *delta, void *stream);

/* A supervised fit of that value MLP: one weight update that regresses given
 * records onto given float targets -- playout means,
 * lookahead values, anything a caller can compute for a position.  Stateless:
 * a device, no handle.  records u32[n][8], 16-B aligned, in the layout the
 * records rollouts and narde_state_records write; target f32[n] white's value
 * to regress to; weight f32[n] or NULL (all 1).  Under the weights as they
 * are on entry:
 *   v_i = v(records[i]), white's value, written to v f32[n] if not NULL;
 *   weight NULL: e_i = target_i - v_i (one float subtraction), G_i = e_i;
 *   weight given: G_i = 0 exactly where w_i == 0 -- target_i is then never
 *                 read and may be NaN --, w_i * e_i elsewhere;
 * then theta += alpha * sum_i G_i * grad_theta v(records[i]) into w1t, b1, w2,
 * b2 and the mirror, the same bits to both: a sum, not a mean.  alpha == 0
 * with finite inputs leaves every weight bit as it was (a validation loss).
 * loss f64[2] (8-B aligned) or NULL = {sum w_i e_i^2, sum w_i}: per slab, in
 * sample order, in double -- (double)w * (double)e * (double)e, w = 1 without
 * weights, a zero-weight sample adding nothing --, then the slabs in slab
 * order.
 * The gradient sum has narde_value_td_window's order and no float atomics --
 * the samples in index order in slabs of NARDE_VALUE_FIT_SLAB
 * (= NARDE_TD_WINDOW_SLAB), every element of a slab's partial row taking its
 * addends in sample order, then the partial rows in slab order --: the same
 * inputs give the same bits, and a window whose every ply is terminated gives
 * narde_value_td_window's bits when its outcomes are the targets.  One
 * forward a sample: no values pass, no returns pass, no v or G read back.
 * scratch: device memory, 16-B aligned, scratch_floats >=
 * NARDE_VALUE_FIT_SCRATCH_FLOATS(n, hidden): a partial row and two doubles a
 * slab, nothing per sample; its contents on return are unspecified.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable once
 * the device has seen one call (the first announces the gradient kernel's
 * LDS).  NARDE_EINVAL before any device call: narde_value_td_trace's net
 * cases, a NULL net, records, target or scratch, a negative device, n < 1 or
 * n >= 2^31, records or scratch not 16-B aligned, scratch too small, loss not
 * 8-B aligned.
 *
 * narde_playout_targets: a playout call's sums i32[n][4] (and its leaf
 * f32[n][trials], or NULL) as regression targets, by narde_playout_pick's
 * score arithmetic (the same bits).  Per root: leaf NULL -- target =
 * (float)((double)points / finished) and weight 1, or target 0 and weight 0
 * when no trial finished; leaf given -- target = (float)(((double)points + S)
 * / trials), S the non-NaN leaves added in trial order in double, weight 1.
 * roots u32[n][8] (16-B aligned) or NULL: a root in which a side already has
 * its 15 checkers off -- a terminal row's record, the none record -- is no
 * position of a game and gets target 0, weight 0.  NARDE_EINVAL before any
 * device call: a NULL sums, target or weight, a negative device, n < 1 or
 * n >= 2^31, trials < 1, n * trials >= 2^31, roots not 16-B aligned. */
#define NARDE_VALUE_FIT_SLAB NARDE_TD_WINDOW_SLAB
#define NARDE_VALUE_FIT_SCRATCH_FLOATS(n, hidden)                                      \
  ((((int64_t)(n) + NARDE_VALUE_FIT_SLAB - 1) / NARDE_VALUE_FIT_SLAB) *                \
   (200 * (int64_t)(hidden) + 4 + 4))
int narde_value_fit(int device, const narde_value_mlp_train *net, int64_t n, const void *records,
                    const float *target, const float *weight, float alpha, float *scratch,
                    int64_t scratch_floats, float *v, double *loss, void *stream);
int narde_playout_targets(int device, int64_t n, int trials, const int32_t *sums, const float *leaf,
                          const void *roots, float *target, float *weight, void *stream);

/* The gradient forms of the two batch updates:
 * narde_value_td_window and narde_value_fit without alpha and with one more
 * output.  grad f32[P], P = 200 * hidden + 1, 16-B aligned, a trace row's
 * layout (above): grad[c * hidden + h] for column c < 198, then b1's, w2's,
 * b2's.  grad[p] is exactly the sum the plain call multiplies by alpha -- the
 * slabs' partial rows added in slab order, from 0.0f --: the direction the
 * plain update moves along, theta += alpha * grad.  Neither the weights nor
 * the mirror are written; v, G, delta and loss come out with the plain call's
 * bits; the scratch macros are the plain calls'.  narde_value_sgd_step with
 * scale == NULL behind one of these leaves the plain call's weight bits.
 * Stream-ordered, allocates nothing, no synchronise, graph-capturable once the
 * device has seen one call.  NARDE_EINVAL before any device call: the plain
 * call's cases, grad NULL or not 16-B aligned. */
int narde_value_td_window_grad(narde_env *env, const narde_value_mlp_train *net, int plies,
                               const void *records, const int32_t *reward, const uint8_t *terminated,
                               const uint8_t *truncated, float lam, float gamma, float *scratch,
                               int64_t scratch_floats, float *delta, float *grad, void *stream);
int narde_value_fit_grad(int device, const narde_value_mlp_train *net, int64_t n, const void *records,
                         const float *target, const float *weight, float *scratch,
                         int64_t scratch_floats, float *v, double *loss, float *grad, void *stream);

/* Optimiser steps on a given gradient f32[P] in that layout (the calls above
 * make one; a caller may average it over ranks or edit it first).  Stateless:
 * a device, no handle.  All three are stream-ordered, allocate nothing, do not
 * synchronise and are graph-capturable; none uses a float atomic, so the same
 * inputs give the same bits.
 *
 * narde_value_grad_norm: out[0] = the Euclidean norm of grad, out[1] =
 * min(1, max_norm / (out[0] + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s
 * coefficient.  One workgroup; the squares are added in double in one fixed
 * order, the norm rounded to float once, the coefficient formed in float.
 *
 * narde_value_sgd_step: theta[p] = fmaf(alpha, g, theta[p]) into w1t, b1, w2,
 * b2 and the mirror (the same bits to both); g = grad[p] when scale is NULL,
 * scale[0] * grad[p] otherwise -- scale a DEVICE float, out + 1 of the norm
 * call for a clipped step.
 *
 * narde_value_adam_step: torch.optim.AdamW(maximize=True) on the row (the
 * papers' Adam is weight_decay = 0).  m and s f32[P], the moments, and state,
 * a narde_adam_state, are the caller's device memory, all zero bytes before
 * the first step.  A call advances state on the device -- step += 1, the
 * running products beta1^t and beta2^t in double (in float32 1 - beta2^t
 * loses about four digits in the first steps) -- in a one-thread launch in
 * front of the element kernel, so a captured graph replays successive steps.
 * Then per element, g as above:
 *   theta *= 1 - lr * weight_decay
 *   m = beta1 * m + (1 - beta1) * g;  s = beta2 * s + (1 - beta2) * g * g
 *   theta += (lr / (1 - beta1^t)) * m / (sqrt(s) / sqrt(1 - beta2^t) + eps)
 * the two bias corrections formed in double and rounded to float once.
 *
 * NARDE_EINVAL before any device call: a negative device, a NULL grad, out,
 * net, weight array, m, s or state, grad, m or s not 16-B aligned, out or
 * scale not 4-B aligned, state not 8-B aligned, hidden outside
 * 1..NARDE_VALUE_HIDDEN_MAX, the net cases of narde_value_td_trace, beta1 or
 * beta2 outside [0, 1), eps <= 0, a negative (or NaN) max_norm, alpha, lr or
 * weight_decay. */
typedef struct narde_adam_state {
  int64_t step;     /* the steps taken */
  double beta1_pow; /* beta1^step */
  double beta2_pow; /* beta2^step */
} narde_adam_state;
int narde_value_grad_norm(int device, int hidden, const float *grad, float max_norm, float *out,
                          void *stream);
int narde_value_sgd_step(int device, const narde_value_mlp_train *net, const float *grad,
                         const float *scale, float alpha, void *stream);
int narde_value_adam_step(int device, const narde_value_mlp_train *net, const float *grad,
                          const float *scale, float *m, float *s, narde_adam_state *state, float lr,
                          float beta1, float beta2, float eps, float weight_decay, void *stream);

/* Masked epsilon-greedy over the 576 codes (the policy of
 * train_deepq_pytorch.py:411-600, batched; stateless): q f32[n][ldq]
 * (ldq >= 576) Q-values, mask u64[n][9] legal codes (the two mask entry
 * points above).  out i64[n] = the legal code with the largest Q (lowest
 * code on ties, as torch.argmax), or with probability epsilon a legal code
 * uniformly at random, or 0 when none is legal.  Draws are Philox4x32-10
 * ({tag, row, 0, 5}, seed); the explore decision depends only on (seed, tag,
 * row), so both heads of one step called with the same tag explore together
 * (head 0 / 1 select independent picks). */
int narde_policy_masked_argmax576(int device, const float *q, int64_t ldq, const uint64_t *mask,
                                  int64_t n, float epsilon, uint64_t seed, uint32_t tag, int head,
                                  int64_t *out, void *stream);

/* The same with epsilon (f32) and tag (int64, low 32 bits used) read from
 * DEVICE memory at run time, so a captured hipGraph replays with the values
 * current at each replay (the DQN driver's decaying epsilon and step tag).
 * Optional addend: with add_tab != NULL the greedy value of code c is
 * q[i][c] + add_tab[add_row[i] * ld_add + c] -- the move-2 head's one-hot
 * column (W[:, 256 + move1], pre-transposed into rows) fused into the
 * argmax instead of materialising a second (n, 576) matrix. */
int narde_policy_masked_argmax576_dev(int device, const float *q, int64_t ldq, const uint64_t *mask,
                                      int64_t n, const float *epsilon, uint64_t seed,
                                      const int64_t *tag, int head, const float *add_tab,
                                      int64_t ld_add, const int64_t *add_row, int64_t *out,
                                      void *stream);

/* narde_policy_masked_argmax576_dev with the head computed inside, for the
 * legal codes only: q_c = f[row] . w[c][0:256] + bias[c] (+ addcol[c * ldw +
 * add_row[row]] when addcol is given: the move-2 head's one-hot column of
 * DecomposedDQN, train_deepq_pytorch.py:184-277), masked argmax (first
 * maximum in code order) or epsilon exploration (the same draws as
 * narde_policy_masked_argmax576_dev).  f f32[B][ldf] (feat = 256), w
 * f32[576][ldw], rows 16-B aligned.  The fp32 sums round differently from a
 * dense GEMM's; a greedy pick can differ only between codes whose Q-values
 * tie to rounding.  The codes go to out[row * ld_out] (i64) and, if out16 is
 * given, out16[row * ld_out16] (i16): straight into a column of the (B, 2)
 * action rows; add_row is read as add_row[row * ld_row]. */
int narde_head_policy576_dev(int device, const float *f, int64_t ldf, int64_t feat, const float *w,
                             int64_t ldw, const float *bias, const uint64_t *mask, int64_t n,
                             const float *epsilon, uint64_t seed, const int64_t *tag, int head,
                             const float *addcol, const int64_t *add_row, int64_t ld_row,
                             int64_t *out, int64_t ld_out, int16_t *out16, int64_t ld_out16,
                             void *stream);

/* One DQN transition for all B envs, fused (the batched trainer of
 * gym_narde/dqn.py, config 4; reward shaping as train_deepq_pytorch.py:
 * 885-912).  After a narde_step: s' = the Tesauro-198 observation of each
 * env's record; r' = reward (+ shaping if `shaping`: for the player the
 * trainer names after the step -- at a step that ended the game the winner
 * (15 off) or, truncated, the other player of the pre-step record -- +1 per
 * checker newly borne off since its off_seen tracker and +0.1 x its off
 * count; none when list #1 was empty; trackers f32[B][2] updated, zeroed on
 * done); done = terminated | truncated.
 *   legal u64[B]: the step's compact list #1 (NULL = every env could move);
 *   misc i32[B]: off_white | off_black << 4 | black_to_move << 10 of each
 *     env before the step on entry (the caller seeds it once from
 *     narde_get_state), after it on return.
 * Replay ring (capacity rows, capacity >= 2B): row j holds transition j's
 * observation s, and s' is row (j + B) % capacity.  This step's transitions
 * are rows (pos + i) % capacity -- their s must already be there -- and get
 * (actions[i], r', done) and priority *max_prio; s' goes to row
 * (pos + B + i) % capacity, whose priority becomes 0 until the next step
 * completes it; state[i] <- s'.  state f32[B][198] out, actions i64[B][2],
 * reward i32[B], terminated/truncated u8[B]; r_obs f32[capacity][198],
 * r_action i64[capacity][2], r_reward/r_done/r_prio f32[capacity]; max_prio
 * f32 and pos i64 are device scalars, 0 <= *pos < capacity (the caller
 * advances pos by B).  B * 198 < 2^31. */
int narde_dqn_transition(narde_env *env, float *state, const int64_t *actions,
                         const int32_t *reward, const uint8_t *terminated,
                         const uint8_t *truncated, const uint64_t *legal, int32_t *misc,
                         float *off_seen, int shaping, float *r_obs, int64_t *r_action,
                         float *r_reward, float *r_done, float *r_prio, const float *max_prio,
                         const int64_t *pos, int64_t capacity, void *stream);

/* ---- DQN learner (gym-narde_amd/csrc/dqn_learner.hip; config 4) ---------
 * The non-GEMM chains of train_deepq_pytorch.py's replay() (:602-750) and
 * PrioritizedReplayBuffer (:279-342) at batch scale, fp32, each one kernel.
 * Device scalars (counter i64, beta f64, max_prio / epsilon f32) are read
 * and updated in place, so the calls can be captured in a graph. */

/* Prioritized sample of `batch` rows from p f32[n] (priority^alpha) and its
 * inclusive prefix sum cdf f32[n]: u_j = Philox4x32-10({*counter, j, 0, 7},
 * seed) (24-bit uniform, written to u if non-NULL), idx_j = first k with
 * cdf[k] > u_j * cdf[n-1] (clamped to n-1), w_j = (n p[idx_j] /
 * cdf[n-1])^-beta / max_j; then beta = min(1, beta + beta_inc), counter += 1.
 * scratch: unused (may be NULL; kept for the ABI).  Two
 * launches: a 64-ary search, one wave per sample, then the normalisation. */
int narde_per_sample(int device, const float *p, const float *cdf, int64_t n, int64_t batch,
                     uint64_t seed, int64_t *counter, double *beta, double beta_inc, int64_t *idx,
                     float *w, float *u, uint32_t *scratch, void *stream);

/* narde_per_sample's inputs from the priorities prio f32[n] (round 6): p =
 * prio^alpha (powf) and cdf = its inclusive prefix sum, in chunks of 1,024
 * rows (chunk f32[chunks] scratch, chunks >= ceil(n / 1024): each chunk's
 * total, then each chunk's rows scanned on top of the totals before it) --
 * the same order on every run; replaces `prio ** alpha` + torch.cumsum
 * (train_deepq_pytorch.py:279-342's probabilities).  prio, p, cdf 16-byte
 * aligned.  Two launches. */
int narde_per_prefix(int device, const float *prio, int64_t n, double alpha, float *p, float *cdf,
                     float *chunk, int64_t chunks, void *stream);

/* Minibatch rows idx i64[batch] of the replay ring (narde_dqn_transition's
 * layout): s = obs[idx], ns = obs[(idx + next_stride) % capacity] (f32
 * [batch][state_size]), a i64[batch][2], r/d f32[batch]. */
int narde_gather_batch(int device, const int64_t *idx, int64_t batch, int state_size,
                       const float *obs, int64_t next_stride, int64_t capacity,
                       const int64_t *action, const float *reward, const float *done, float *s,
                       float *ns, int64_t *a, float *r, float *d, void *stream);

/* out[i] = max_c base[i][c] + tab[rows[i]][c] over the 576 codes (the target
 * move-2 head's max with its one-hot column added on the fly). */
int narde_rowmax_addend(int device, const float *base, int64_t ld, const float *tab,
                        int64_t ld_tab, const int64_t *rows, int64_t n, float *out, void *stream);

/* The online network's two heads (DecomposedDQN.move1_head / move2_head,
 * train_deepq_pytorch.py:184-222) at the stored codes only -- what the loss
 * of train_deepq_pytorch.py:653-720 reads (q.gather(1, action)):
 *   q1[i] = f[i] . w1[a1] + b1[a1],
 *   q2[i] = (f[i] . w2[a2][:256] + b2[a2]) + w2[a2][256 + a1]
 * with (a1, a2) = a[i][0..1] (i64; codes clamped to 0..575), f f32[n][ldf]
 * (256 features), w1 f32[576][ldw1 >= 256], w2 f32[576][ldw2 >= 832] (the
 * move-2 head's weight: 256 feature columns, then 576 one-hot columns);
 * f, w1, w2 16-byte aligned, leading dimensions multiples of 4. */
int narde_dqn_heads_forward(int device, const float *f, int64_t ldf, const float *w1,
                            int64_t ldw1, const float *b1, const float *w2, int64_t ldw2,
                            const float *b2, const int64_t *a, int64_t n, float *q1, float *q2,
                            void *stream);

/* The backward of narde_dqn_heads_forward for dloss/dq1 = g1, dloss/dq2 = g2
 * (f32[n]): gf f32[n][256] (dense, 16-byte aligned), and the heads' whole
 * gradients gw1 f32[576][256], gb1 f32[576], gw2 f32[576][832], gb2
 * f32[576] (every element written; zero for codes no row holds).  Each sum
 * runs in a fixed order: deterministic. */
int narde_dqn_heads_backward(int device, const float *g1, const float *g2, const float *f,
                             int64_t ldf, const float *w1, int64_t ldw1, const float *w2,
                             int64_t ldw2, const int64_t *a, int64_t n, float *gf, float *gw1,
                             float *gb1, float *gw2, float *gb2, void *stream);

/* The backward of h = relu(x W^T + b) up to the weight GEMM (the learner's
 * feature layers, train_deepq_pytorch.py:184-201): g = gh * (h > 0) and db =
 * the column sums of g, for gh, h, g f32[n][cols] (cols <= 4096).
 * scratch: f32[ceil(n / 64) * cols] of device memory.  Deterministic. */
int narde_relu_bias_grad(int device, const float *gh, const float *h, int64_t n, int64_t cols,
                         float *g, float *db, float *scratch, void *stream);

/* torch.nn.utils.clip_grad_norm_(max_norm) + one torch.optim.Adam step
 * (train_deepq_pytorch.py's optimizer) over n_tensors <= 8 fp32 parameter
 * tensors (params/grads/m/v: arrays of n_tensors device pointers, sizes in
 * elements).  *step (device i64) is advanced first; scratch: >= 1026 floats
 * of device memory, its last word zero before the first call (left zero).
 * float4 passes when every size is a multiple of 4 and every pointer 16-byte
 * aligned, else one element per thread: the same update either way. */
int narde_adam_clip(int device, int n_tensors, float *const *params, const float *const *grads,
                    float *const *m, float *const *v, const int64_t *sizes, int64_t *step, float lr,
                    float beta1, float beta2, float eps, float max_norm, float *scratch,
                    void *stream);

/* Round 6's one-launch forms of the learner's chains (the calls above stay
 * for the torch-restatement tests):
 * narde_per_sample_gather = narde_per_sample's search + narde_gather_batch's
 * rows in one launch, w UNNORMALISED ((n p / total)^-beta); beta and the
 * counter are NOT stepped (narde_dqn_loss_prio does both). */
int narde_per_sample_gather(int device, const float *p, const float *cdf, int64_t n, int64_t batch,
                            uint64_t seed, const int64_t *counter, const double *beta, int64_t *idx,
                            float *w, int state_size, const float *obs, int64_t next_stride,
                            int64_t capacity, const int64_t *action, const float *reward,
                            const float *done, float *s, float *ns, int64_t *a, float *r, float *d,
                            void *stream);

/* The target heads' maxima: m1[i] = max_c nq1[i][c], am1[i] = its argmax
 * (torch.max(dim): NaN wins, ties to the lowest code; am1 may be NULL),
 * m2[i] = max_c base[i][c] + tab[am1[i]][c] (narde_rowmax_addend's sum). */
int narde_target_max2(int device, const float *nq1, int64_t ld1, const float *base, int64_t ld,
                      const float *tab, int64_t ld_tab, int64_t n, float *m1, int64_t *am1,
                      float *m2, void *stream);

/* The decomposed DQN loss (train_deepq_pytorch.py:653-720) on batch rows and
 * the bookkeeping of one update, in one block: w[j] /= max_j w[j] in place
 * (w raw, from narde_per_sample_gather); t = r + (1 - d) * gamma * m (m1/m2
 * the target heads' maxima), td = clamp(|t1 - q1| + |t2 - q2|, 0, 100),
 * *loss = mean(w (q1 - t1)^2) + mean(w (q2 - t2)^2) (also to *loss_copy if
 * non-NULL), g1/g2 = dloss/dq1, dloss/dq2; prio[idx_j] = td_j + eps,
 * *max_prio = max(*max_prio, max_j); then, if epsilon is non-NULL, *epsilon
 * *= eps_decay when *epsilon > eps_min; if cursor is non-NULL, *cursor =
 * (*cursor + cursor_add) % cursor_mod (the replay ring's write cursor); if
 * tag is non-NULL, *tag += 1 (the driver's step tag); beta = min(1, beta +
 * beta_inc) and *counter += 1 (the sampler's device scalars). */
int narde_dqn_loss_prio(int device, const float *q1, const float *q2, const float *m1,
                        const float *m2, const float *r, const float *d, float *w, int64_t batch,
                        float gamma, float *td, float *loss, float *loss_copy, float *g1, float *g2,
                        const int64_t *idx, float eps, float *prio, float *max_prio, float *epsilon,
                        float eps_min, float eps_decay, int64_t *cursor, int64_t cursor_add,
                        int64_t cursor_mod, int64_t *tag, int64_t *counter, double *beta,
                        double beta_inc, void *stream);

/* Stateless: Narde._violates_block_rule on n perspective boards i8[n][24]. */
int narde_violates_block_rule(int device, const int8_t *boards, int64_t n, uint8_t *out,
                              void *stream);

/* ---- host-memory entry points (scalar facade; synchronous) ----------------
 * Same semantics as above on n <= 4096 envs given explicitly in HOST memory.
 * The handle's own B envs are untouched.  Return NARDE_EINVAL for an invalid
 * position (see narde_set_state). */
int narde_host_legal_moves(narde_env *env, int64_t n, const int8_t *board, const uint8_t *off,
                           const uint8_t *first_turn, const int8_t *player, const uint8_t *dice4,
                           int16_t *count, int8_t *moves);
int narde_host_step(narde_env *env, int64_t n, int8_t *board, uint8_t *off, uint8_t *first_turn,
                    int8_t *player, const uint8_t *dice2, const int16_t *actions, int32_t *obs,
                    int32_t *reward, uint8_t *terminated);
int narde_host_apply_moves(narde_env *env, int64_t n, int8_t *board, uint8_t *off,
                           uint8_t *first_turn, const int8_t *player, const int8_t *moves);
int narde_host_violates_block_rule(narde_env *env, int64_t n, const int8_t *boards, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* NARDE_H */
