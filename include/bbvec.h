/*
 * bbvec.h -- C-ABI of the MI355X-native Block Blast vectorised environment and
 * masked-PPO rollout kernels (libbbvec.so, gfx950).
 *
 * This is the drop-in boundary under the reference's Python surface
 * (SURVEY.md section 8(b)).  The reference has no FFI of its own; each entry
 * point below names the reference interface it replaces, and INTEGRATION.md
 * shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch types.  "d_" pointers are device
 *     (HBM) pointers owned by the caller (e.g. tensor.data_ptr()); "h_" are host.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     launches are asynchronous on that stream; nothing allocates or syncs
 *     inside bb_step / bb_obs / bb_masked_sample / bb_gae (graph-capturable).
 *   - Return value: 0 = BB_OK, negative = error; bb_last_error() explains.
 *     An invalid *action* is not an error: it is reproduced in-kernel as the
 *     reference does (reward -10, no state change; block_blast_env.py:240-245).
 *   - A handle is single-stream and not re-entrant (the reference is
 *     single-threaded).  Multi-GPU = one handle per process/device.
 *
 * Mask bit layout (shared by every entry point): uint64 mask[N][3], word p is
 * piece slot p, bit (r*8+c) set iff placing slot p at (r,c) is legal; flat
 * action a = p*64 + r*8 + c (block_blast_env.py:104-132).
 */
#ifndef BBVEC_H
#define BBVEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BB_ABI_VERSION 9  /* 2: bb_step_out.final_score / final_moves; 3: bb_sync, BB_ERR_DEVICE;
                              4: bb_conv_in_* and bb_relu_bias_grad* removed;
                              5: bb_conv3x3_forward_stats / _stats_parts and bb_bn_forward_parts removed;
                              6: bb_build_id; bb_obs / bb_snapshot report BB_ERR_DEVICE;
                                 bb_conv3x3_f32_prep / _forward, bb_linear_f32;
                              7: bb_ppo_loss_forward_bf16 / _backward_bf16;
                              8: bb_dropout_forward, bb_linear_bgrad, bb_linear_wgrad, bb_linear_n1_*;
                                 bb_conv_in_forward / _wgrad; bb_bn_backward_res; bb_ppo_loss_fused and the
                                 loss forward's d_cnt (one launch, the statistics finalised in it);
                                 bb_conv3x3_wgrad_partial / _reduce / _chunks, bb_bn_backward_red,
                                 bb_conv_in_forward_prep, bb_linear_bgrad2, bb_conv3x3_forward_stats,
                                 bb_conv3x3_stats_blocks, bb_bn_forward_part, bb_conv3x3_forward_bstats,
                                 bb_bn_backward_part;
                                 (additive, still 8) bb_positions / bb_afterstate_out / bb_greedy_weights with
                                 bb_afterstates(_pos) and bb_greedy_actions(_pos): one-ply lookahead
                                 (engine.py:326-346, 390-454; block_blast_env.py:148-193);
                                 (additive, still 8) bb_plan_out with bb_plan_actions(_pos): full-hand lookahead;
                              9: bb_bn_fwd / bb_bn_bwd / bb_wgrad_reduce / bb_ppo_loss_args: bb_bn_forward, bb_bn_backward
                                 and bb_ppo_loss_forward / _backward / _fused take one argument struct;
                                 bb_bn_forward_res / _part, bb_bn_backward_red / _part / _res and
                                 bb_ppo_loss_forward_bf16 / _backward_bf16 removed (fields of the structs);
                                 (additive, still 9) bb_plan_values_out with bb_plan_values(_pos): per-action
                                 full-hand values and the hand-safe mask;
                                 (additive, still 9) bb_safe_mask(_pos): the hand-safe mask alone, by an
                                 existence search, and the sampling mask (safe, else legal);
                                 (additive, still 9) bb_distill_loss_args with bb_distill_loss_forward / _backward /
                                 _fused: policy distillation from the search values; bb_snapshot_combo;
                                 (additive, still 9) bb_guided_loss_args with bb_guided_loss_forward / _backward /
                                 _fused: the PPO loss and the distillation cross-entropy on one softmax;
                                 (additive, still 9) bb_greedy_actions_each(_pos) and bb_plan_actions_each(_pos): one
                                 row of weights per position, read from the memory of the position columns;
                                 (additive, still 9) bb_census_out with bb_refill_census(_pos): the exact count of
                                 the 37^3 hands a board can still be dealt (engine.py:155-224);
                                 (additive, still 9) bb_refill_values_out with bb_refill_values(_pos): next hands
                                 dealt by the dealer's law (engine.py:155-172) and searched, per board; bb_play_plan_out
                                 with bb_play_plan_pos: a plan played to its leaf position;
                                 (additive, still 9) bb_eval_weights with bb_board_terms(_pos) and
                                 bb_plan_actions_ext(_pos): four shape terms of a board (perimeter, room3, room5,
                                 fits) and the full-hand search with them added to every leaf's value;
                                 (additive, still 9) bb_plan_values_ext(_pos) and bb_refill_values_ext(_pos): the
                                 per-action values and the dealt next-hand values under rows of bb_eval_weights;
                                 (additive, still 9) bb_plan2_out with bb_plan2_values(_pos) and bb_plan2_work_bytes:
                                 the two-hand decision (values, candidates, leaves, deals, choice) in one call;
                                 (additive, still 9) bb_playout_out with bb_playout_values(_pos): the plan agent
                                 played for several dealt hands past the refill, in one launch */

#define BB_OK 0
#define BB_ERR_ARG (-1)
#define BB_ERR_HIP (-2)
#define BB_ERR_STATE (-3)
#define BB_ERR_DEVICE (-4) /* a kernel reported a failure through the handle's status word */

#define BB_NUM_PIECES 37
#define BB_ACTIONS 192

typedef struct bb_env bb_env;

/* Reward weights: block_blast_env.py:63-73 (defaults), overridable from the
 * YAML `rewards:` section exactly like reward_config.update(). */
typedef struct bb_reward_cfg {
  double line_clear_base;        /* 1.0   */
  double block_placed;           /* 0.01  */
  double game_over_penalty;      /* -1.0  */
  double hole_penalty;           /* -0.05 */
  double center_bonus;           /* 0.02  */
  double combo_multiplier_bonus; /* 0.5   */
  double survival_bonus;         /* 0.001 */
} bb_reward_cfg;

/* Per-env info record written by bb_step (optional output).  Mirrors the
 * `info` dict of block_blast_env.py:266-288 (values AFTER the move, BEFORE any
 * auto-reset) plus the terminal-observation latch of wrappers.py:97-102. */
typedef struct bb_info {
  int64_t score;          /* info['score'] (== info['final_score'] on termination) */
  int64_t score_gained;   /* info['last_move']['score_gained'] */
  uint64_t term_board;    /* board bits before auto-reset (terminal_observation) */
  int32_t moves;          /* info['moves'] */
  int32_t lines;          /* info['lines_cleared'] (total) */
  int32_t max_combo;      /* info['max_combo'] */
  int32_t blocks;         /* info['blocks_placed'] (total) */
  uint32_t term_hand;     /* packed hand word before auto-reset (see bb_state) */
  uint8_t holes;          /* info['holes'] */
  uint8_t filled;         /* popcount(board): info['board_fill'] = filled / 64 */
  uint8_t flags;          /* bit0 invalid_action, bit1 terminated, bit2 has last_move */
  uint8_t last_blocks;    /* info['last_move']['blocks_placed'] */
  uint8_t last_lines;     /* info['last_move']['lines_cleared'] */
  uint8_t last_cm;        /* info['last_move']['combo_multiplier'] */
  uint8_t pad[2];
} bb_info;

/* Outputs of one bb_step.  reward and terminated are required, the rest may be
 * NULL.  `next_action`, when non-NULL, runs the fused synthetic random policy
 * (BASELINE config 2): for every env, u = Philox4x32-10(key=policy_seed,
 * ctr=(env_offset+i, policy_step)).x, k = (u * popcount(mask)) >> 32, and the
 * action is the k-th set bit of the post-step 192-bit mask (0 if empty). */
typedef struct bb_step_out {
  float* reward;          /* [N] f32 (wrappers.py:88,105)                       */
  uint8_t* terminated;    /* [N] 0/1; truncated is always false                  */
  double* reward_f64;     /* [N] optional: the fp64 reward BlockBlastEnv returns */
  uint64_t* mask;         /* [N][3] optional: post-step (post-reset) mask bits   */
  uint8_t* lines;         /* [N] optional: lines cleared by this move            */
  bb_info* info;          /* [N] optional                                        */
  int32_t* next_action;   /* [N] optional: fused random policy for the next step */
  uint64_t policy_seed;
  uint64_t policy_step;
  uint64_t env_offset;    /* global index of env 0 (multi-GPU shards)            */
  int64_t* final_score;   /* [N] optional: written ONLY for envs that terminated:
                             the episode's score before the auto-reset
                             (info['final_score'], wrappers.py:97-101)          */
  int32_t* final_moves;   /* [N] optional: likewise its moves (info['moves'];
                             scripts/train.py:196-201 reads both)               */
} bb_step_out;

/* Host view of the packed per-env state (bb_get_state / bb_set_state).
 * hand word: bits 0-5 slot0 piece id, 6-11 slot1, 12-17 slot2, 18-20 used,
 * 21 game_over, 22 pcg has_uint32.  Any pointer may be NULL (skipped). */
typedef struct bb_state_view {
  uint64_t* board;        /* [N] bit r*8+c = grid[r][c]                    */
  uint32_t* hand;         /* [N] packed hand word                           */
  int64_t* score;         /* [N]                                            */
  int32_t* combo;         /* [N] combo_count (engine.py:115)                */
  int32_t* max_combo;     /* [N]                                            */
  int32_t* moves;         /* [N]                                            */
  int32_t* lines;         /* [N] total_lines_cleared                        */
  int32_t* blocks;        /* [N] total_blocks_placed                        */
  uint8_t* prev_holes;    /* [N] BlockBlastEnv._prev_holes                  */
  uint8_t* prev_center;   /* [N] filled centre cells behind _prev_center_openness */
  uint64_t* rng;          /* [N][3] pcg state hi, state lo, uinteger        */
} bb_state_view;

/* ---- lifetime -------------------------------------------------------------
 * bb_create replaces VectorizedBlockBlastEnv.__init__ (wrappers.py:21-51) /
 * BlockBlastEnv.__init__ (block_blast_env.py:42-102).  autoreset=1 gives the
 * vec-env semantics (wrappers.py:97-102), 0 the single-env semantics.  The new
 * envs are unseeded until bb_seed + bb_reset. */
int bb_abi_version(void);
/* The id of the sources this library was built from: the first 16 hex digits of a SHA-256 over csrc/,
 * include/bbvec.h and the compiler flags (runtime/build.py source_id).  runtime/lib.load() refuses a
 * library whose id is not that of the sources beside it.  No reference counterpart. */
const char* bb_build_id(void);
int bb_create(int32_t num_envs, int32_t device, const bb_reward_cfg* cfg,
              int32_t autoreset, bb_env** out);
void bb_destroy(bb_env* env);
const char* bb_last_error(const bb_env* env); /* env may be NULL (last create error) */
int32_t bb_num_envs(const bb_env* env);

/* numpy-exact default_rng(seed) initialisation: SeedSequence(seed)
 * .generate_state(4, uint64) -> PCG64 set_seed.  out = {state_hi, state_lo,
 * inc_hi, inc_lo}.  Replaces np.random.default_rng (engine.py:109,138). */
int bb_pcg64_seed(uint64_t seed, uint64_t out[4]);

/* Per-env seeding (host arrays of length N).
 *   has_seed[i] == 1: seeded from seeds[i] (numpy default_rng(seeds[i])) now
 *     AND on every later reset -- the reference re-seeds each episode with
 *     seed_value (block_blast_env.py:212-215, engine.py:137-138);
 *   has_seed[i] == 2: same, but the post-seeding PCG64 words come from
 *     raw[i*4..i*4+3] = {state_hi, state_lo, inc_hi, inc_lo} (seeds that do
 *     not fit uint64, computed by the caller);
 *   has_seed[i] == 0: raw words (e.g. fresh OS entropy) and the stream
 *     continues across resets (seed_value None).
 * raw may be NULL when every has_seed is 1. */
int bb_seed(bb_env* env, const uint64_t* h_seeds, const uint8_t* h_has_seed,
            const uint64_t* h_raw);

/* Reset envs (all when d_env_mask is NULL, else those with mask[i] != 0):
 * engine.py:127-153 + block_blast_env.py:195-222. */
int bb_reset(bb_env* env, const uint8_t* d_env_mask, void* stream);

/* One step of every env with actions d_actions[N] (int32 flat actions):
 * VectorizedBlockBlastEnv.step (wrappers.py:75-116) -> BlockBlastEnv.step
 * (block_blast_env.py:224-264) -> GameEngine.make_move (engine.py:390-454).
 * If a launch fails, the handle refuses bb_step / bb_rollout / masked
 * bb_reset with BB_ERR_STATE until a full bb_reset (d_env_mask NULL): the
 * step kernel may already have parked envs whose search never ran. */
int bb_step(bb_env* env, const int32_t* d_actions, const bb_step_out* out,
            void* stream);

/* T steps of every env in ONE launch under the fused synthetic random policy
 * (BASELINE config 2; the reference's rollout loop of wrappers.py:128-137
 * sample_valid_actions -> wrappers.py:75-116 step, with the Philox policy of
 * bb_step_out.next_action in place of np.random.choice).  Output for output
 * and in the final state it equals T chained bb_step calls: call t takes
 * d_actions (t = 0) or call t-1's next_action, with policy_step =
 * policy_step0 + t + 1.  Per-step outputs are [T][N] (t-major); the env
 * state stays in registers between steps, so nothing but these outputs
 * touches HBM inside the rollout. */
typedef struct bb_rollout_out {
  float* reward;          /* [T][N] f32, required                             */
  uint8_t* terminated;    /* [T][N] 0/1, required                             */
  uint8_t* lines;         /* [T][N] optional: lines cleared by each move      */
  int32_t* actions;       /* [T][N] optional: the action applied at step t    */
  uint64_t* mask;         /* [T][N][3] optional: post-step (post-reset) masks */
  int32_t* next_action;   /* [N] optional: policy action after the last step  */
  uint64_t policy_seed;
  uint64_t policy_step0;
  uint64_t env_offset;    /* global index of env 0 (multi-GPU shards)         */
} bb_rollout_out;

int bb_rollout(bb_env* env, int32_t steps, const int32_t* d_actions,
               const bb_rollout_out* out, void* stream);

/* Device-side failures.  The rollout kernel bounds its own iterations so that
 * a logic error can never hang the GPU; if a bound is ever hit it writes the
 * handle's status word instead of failing silently.  Every later bb_step /
 * bb_rollout / bb_get_state / masked bb_reset then returns BB_ERR_DEVICE
 * (bb_last_error says which kernel and why) until a full bb_reset (d_env_mask
 * NULL).  Launches are asynchronous, so the check at the next call sees only
 * the launches that have finished by then; bb_sync waits for every launch on
 * `stream` and reports their status (BB_OK or BB_ERR_DEVICE / BB_ERR_HIP).
 * The reference has no device side; this replaces the exceptions its Python
 * step loop would raise (wrappers.py:75-116). */
int bb_sync(bb_env* env, void* stream);

/* Observation expansion (engine.py:478-507, block_blast_env.py:134-146,
 * wrappers.py:118-126).  Any output may be NULL:
 *   d_x      [N][4][8][8] f32: plane 0 board, planes 1-3 unused piece shapes
 *   d_mask_i8  [N][192] int8,  d_mask_f32 [N][192] f32,  d_mask_bits [N][3]. */
int bb_obs(bb_env* env, float* d_x, int8_t* d_mask_i8, float* d_mask_f32,
           uint64_t* d_mask_bits, void* stream);

/* Device pointers of the live state columns (board [N], hand [N], mask
 * [N][3]) for zero-copy snapshots into a device rollout buffer.  Valid until
 * bb_destroy; read them on the stream that runs bb_step. */
int bb_device_ptrs(bb_env* env, uint64_t** d_board, uint32_t** d_hand, uint64_t** d_mask);

/* Async device-to-device snapshot of the packed observation state into caller
 * buffers (the packed rollout-buffer record, ppo.py:100-102 without the f32
 * planes): board [N] u64, hand [N] u32, mask [N][3] u64.  Any may be NULL. */
int bb_snapshot(bb_env* env, uint64_t* d_board, uint32_t* d_hand, uint64_t* d_mask_bits, void* stream);

/* Async device-to-device copy of the live combo column into d_combo [N] i32:
 * with bb_snapshot's board and hand a stored position that bb_plan_values_pos
 * can search later (plan values carry the score along the sequence, which
 * reads combo; prev is read by the afterstate reward only).  Handle checks and
 * errors are bb_snapshot's. */
int bb_snapshot_combo(bb_env* env, int32_t* d_combo, void* stream);

/* Synchronous state copies (tests / info / checkpoint).  bb_set_state also
 * overwrites the pcg state when v->rng is given. */
int bb_get_state(bb_env* env, const bb_state_view* h_view);
int bb_set_state(bb_env* env, const bb_state_view* h_view);

/* Diagnostics: per-env hand-search counters of the last bb_step, [N][4] =
 * {in-lane cycles, attempts | escalated << 32, wave cycles, board}.  Only
 * available when the env was created with BB_DEBUG_MODE having bit 1 set;
 * reading clears them.  NOTE: BB_DEBUG_MODE bit 1 (value 2) also switches the
 * escalate kernel from the shipped multi-env search (gen_hands_multi) to the
 * one-env-at-a-time wave search (gen_hand_wave) that these counters
 * instrument; both are exact (tests/test_gpu_solver_stress.py runs the
 * fallback), but the counters describe the fallback's work, not the shipped
 * path's. */
int bb_debug_counters(bb_env* env, uint64_t* h_out);

/* Synthetic random policy on its own (see bb_step_out.next_action). */
int bb_random_actions(const uint64_t* d_mask_bits, int32_t n, uint64_t seed,
                      uint64_t step, uint64_t env_offset, int32_t* d_actions,
                      void* stream);

/* ---- one-ply lookahead ------------------------------------------------------
 * The deterministic half of a step, for all 192 actions of a position at once
 * and without touching any env: what GameEngine.can_place_piece (engine.py:
 * 326-346) accepts, what GameEngine.make_move (engine.py:390-454) does to the
 * board, combo and score before it draws a new hand, and the reward
 * BlockBlastEnv._calculate_reward (block_blast_env.py:148-193) gives for it.
 * The reference has no such call (it would be copy.deepcopy(env).step(a) for
 * every a); afterstate learning, one-ply policy improvement and tree search
 * start from it.
 *
 * A position is (board, packed hand word as in bb_state_view, combo, prev =
 * prev_holes | filled centre cells << 8).  Action a = p*64 + r*8 + c is legal
 * iff the hand's game-over bit is clear, slot p is unused and the piece fits
 * at (r,c): exactly the actions bb_step accepts.
 *   illegal a: board = the position's board, reward_f64 = -10.0 (block_blast_
 *     env.py:240-245), score_gained = 0, aux = 0.
 *   legal a: board = the board after the piece is placed and every full row
 *     and column (found on the same board) is cleared; lines = rows + cols;
 *     combo' = lines > 0 ? combo + 1 : 0; score_gained = cells + (lines > 0 ?
 *     lines*8*10 * min(lines,4) * min(combo'+1,8) : 0) (engine.py:274-312, 427).
 *     refill = all three slots used after the move: the next hand is a chance
 *     outcome, so whether the game then ends is not reported.  mobility = the
 *     number of legal (slot, r, c) placements of the still-unused slots on the
 *     new board (0 when refill); dead = !refill && mobility == 0, which for a
 *     non-refill move is bb_step's `terminated`.  reward_f64 = _calculate_
 *     reward with game_over = dead, the new board's holes against prev_holes
 *     and its centre cells against prev's, in fp64 in the reference's
 *     operation order with no FMA contraction: bit-equal to bb_step's
 *     reward_f64 for a non-refill move, and for a refill move whenever that
 *     step does not terminate.
 *     aux: bit 0 legal, bit 1 dead, bit 2 refill, bits 8-11 lines, 12-18 holes
 *     of the new board (board.py:195-216), 19-23 its filled centre cells
 *     (rows / cols 2-5, board.py:236-243), 24-31 mobility.
 *     (A position reachable in play clears at most 6 lines with one piece; a
 *     crafted board with more than 15 full lines would not fit the lines
 *     field.  A slot whose piece id is not below BB_NUM_PIECES fits nowhere.)
 * Outputs are [n][192], action-major per position; any may be NULL.  The
 * handle forms read the handle's live columns and reward config and change
 * nothing, the RNG included; like bb_step they refuse a handle in
 * BB_ERR_DEVICE / BB_ERR_STATE.  Asynchronous on `stream`, no allocation, no
 * sync (graph-capturable); indexing is 64-bit. */
typedef struct bb_positions {
  const uint64_t* board;  /* [n] bit r*8+c                                     */
  const uint32_t* hand;   /* [n] packed hand word (bb_state_view)              */
  const int32_t* combo;   /* [n] combo_count, NULL = 0                         */
  const uint16_t* prev;   /* [n] prev_holes | centre cells << 8, NULL = 0      */
} bb_positions;           /* device pointers */

typedef struct bb_afterstate_out {
  uint64_t* board;        /* [n][192] */
  double* reward_f64;     /* [n][192] */
  int32_t* score_gained;  /* [n][192] */
  uint32_t* aux;          /* [n][192] */
} bb_afterstate_out;      /* device pointers, any may be NULL */

/* Weights of the one-ply greedy value, an exact int64 sum (no floats):
 * lines*lines' + score*score_gained + holes*holes' + filled*popcount(board') +
 * centre*centre' + mobility*mobility + dead*dead + refill*refill. */
typedef struct bb_greedy_weights {
  int32_t lines, score, holes, filled, centre, mobility, dead, refill;
} bb_greedy_weights;

int bb_afterstates_pos(const bb_positions* pos, int32_t n, const bb_reward_cfg* cfg, const bb_afterstate_out* out,
                       void* stream);
int bb_afterstates(bb_env* env, const bb_afterstate_out* out, void* stream);
/* The fused consumer: d_action[i] = the legal action of position i with the
 * largest greedy value, ties to the lowest flat action; d_value[i] (NULL ok) =
 * that value.  No legal action: action 0, value INT64_MIN.  One launch, 4 (+8)
 * bytes written per position; the [n][192] arrays are never materialised. */
int bb_greedy_actions_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t* d_action,
                          int64_t* d_value, void* stream);
int bb_greedy_actions(bb_env* env, const bb_greedy_weights* w, int32_t* d_action, int64_t* d_value, void* stream);
/* bb_greedy_actions with one row of weights per position: d_action[i] / d_value[i] are exactly what
 * bb_greedy_actions_pos returns for position i alone with w = d_w[i].  d_w is [n] rows ([num_envs] for the handle
 * form) of eight int32 in the struct's field order; any int32 is a valid weight.  The rows live in the same
 * memory as the position columns: device memory for libbbvec.so, host memory for libbbvec_host.so.  The calls
 * above take w as a host struct; these take d_w as a pointer into that memory, read when the launch runs, so
 * a captured launch replays with whatever the rows hold then.  One launch; refusals, asynchrony, no allocation and
 * graph capture as above (a NULL d_w is refused, and n <= 0 in the _pos form). */
int bb_greedy_actions_each_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* d_w, int32_t* d_action,
                               int64_t* d_value, void* stream);
int bb_greedy_actions_each(bb_env* env, const bb_greedy_weights* d_w, int32_t* d_action, int64_t* d_value, void* stream);

/* ---- full-hand lookahead ----------------------------------------------------
 * The exhaustive search over the deterministic part of a decision: the up to
 * three pieces of the hand (engine.py:155-172 deals them together) may be
 * played in any order and nothing random happens until the third one is placed
 * (engine.py:432-437 draws the next hand only then), so the best way to play
 * the hand out is a plain maximum over move sequences.  The reference has no
 * such call.  Every move is the one-ply move above: legality (engine.py:
 * 326-346), B', lines, combo', score_gained (engine.py:390-431), refill,
 * mobility, dead (engine.py:348-362), holes', centre', filled'.
 *
 * search(P, d), d >= 1: for every legal action a of P with afterstate S, S is
 * terminal if d == 1 or S.refill or S.dead and ends a maximal sequence;
 * otherwise search((S.board, hand with slot p marked used, combo'), d - 1).
 * dead means no unused slot fits anywhere, so a search never meets a position
 * without a move below the root.  The value of a maximal sequence a_1..a_k
 * (k <= depth) under bb_greedy_weights w is the int64 sum
 *   w.lines * sum_j lines_j + w.score * sum_j score_gained_j (combo carried)
 *   + w.holes*holes_k + w.filled*filled_k + w.centre*centre_k
 *   + w.mobility*mobility_k + w.dead*dead_k + w.refill*refill_k
 * with the state terms taken from the last afterstate: at depth 1 the greedy
 * value, term for term.  Per position the maximal sequence with the largest
 * value is returned, ties to the lexicographically lowest (a_1, a_2, a_3).
 *   action [n]    a_1; 0 when the position has no legal action
 *   value  [n]    the best value; INT64_MIN when there is no legal action
 *   plan   [n][3] a_1, a_2, a_3, -1 for plies not played (all -1: no action)
 *   leaves [n]    the number of maximal sequences (<= 192*128*64 = 1,572,864)
 * action is required, the others may be NULL.  depth is 1..3.  The handle form
 * reads the live columns and changes nothing, the RNG included, and refuses a
 * handle in BB_ERR_DEVICE / BB_ERR_STATE.  Asynchronous on `stream`, no
 * allocation, no sync (graph-capturable); indexing is 64-bit. */
typedef struct bb_plan_out {
  int32_t* action;  /* [n]    required */
  int64_t* value;   /* [n]    NULL ok  */
  int32_t* plan;    /* [n][3] NULL ok  */
  int32_t* leaves;  /* [n]    NULL ok  */
} bb_plan_out;      /* device pointers */

int bb_plan_actions_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t depth,
                        const bb_plan_out* out, void* stream);
int bb_plan_actions(bb_env* env, const bb_greedy_weights* w, int32_t depth, const bb_plan_out* out, void* stream);
/* bb_plan_actions with one row of weights per position: position i's action, value, plan and leaves are exactly
 * what bb_plan_actions_pos returns for position i alone with w = d_w[i] (the tie rule, action 0 / INT64_MIN
 * without a legal action, NULL optional outputs, depth 1..3).  d_w is [n] rows ([num_envs] for the handle form)
 * of eight int32 in the struct's field order, in the same memory as the position columns: device memory for
 * libbbvec.so, host memory for libbbvec_host.so -- unlike w above, which is a host struct.  The rows are read when
 * the launch runs.  One launch for a whole population of weight vectors; refusals as bb_plan_actions(_pos), with
 * a NULL d_w refused; asynchronous, no allocation, graph-capturable from the first call. */
int bb_plan_actions_each_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* d_w, int32_t depth,
                             const bb_plan_out* out, void* stream);
int bb_plan_actions_each(bb_env* env, const bb_greedy_weights* d_w, int32_t depth, const bb_plan_out* out, void* stream);

/* ---- shape terms ---------------------------------------------------------------
 * Four exact integer terms of a board B (bit r*8+c set: cell filled).  "Fits" is
 * Board.can_place (board.py:71-93): every cell of the piece on the board and empty.
 *   perimeter  the pairs (empty cell, one of its four sides) whose neighbour across
 *              that side is filled or off the board.  Empty board 32, full board 0.
 *   room3      the anchors at which SQUARE_3x3 (piece 36) fits, 0..36
 *   room5      the anchors at which I5_H (piece 15) fits plus those of I5_V (16), 0..64
 *   fits       the piece ids 0..36 that fit at one anchor or more, 0..37
 * bb_board_terms(_pos) writes them in this order, d_terms[i][0..3], for every board
 * (the handle form: the live boards).  One launch, no allocation, no sync
 * (graph-capturable), 64-bit indexing; n == 0 does nothing.  BB_ERR_ARG (the rule named
 * in bb_last_error, before any HIP call) for a NULL board, n < 0 and a NULL d_terms. */
int bb_board_terms_pos(const uint64_t* d_board, int32_t n, int32_t* d_terms /* [n][4] */, void* stream);
int bb_board_terms(bb_env* env, int32_t* d_terms /* [N][4] */, void* stream);

/* bb_plan_actions with the shape terms in the value: search(P, depth) above, move for
 * move, with the same tie rule, outputs and "no legal action" answer.  The value of a
 * maximal sequence is the sum above plus
 *   w.perimeter*perimeter(B_k) + w.room3*room3(B_k) + w.room5*room5(B_k) + w.fits*fits(B_k)
 * with B_k the board of the last afterstate after its clears, at dead and refill leaves
 * alike.  d_w are rows of twelve int32 in the struct's field order, in the memory of the
 * position columns (device memory for libbbvec.so, host memory for libbbvec_host.so),
 * read when the launch runs.  w_stride 0: every position uses d_w[0]; 1: position i uses
 * d_w[i]; any other value is refused.  A term whose weight is 0 in a position's row is
 * not computed for that position, and with all four 0 the answers are those of
 * bb_plan_actions_each(_pos) for `base`.  BB_ERR_ARG (the rule named, before any HIP
 * call) for NULL positions, n < 0 (n == 0 does nothing), NULL weight rows, a w_stride
 * that is not 0 or 1, depth outside 1..3 and a NULL out or out->action.  The handle form
 * refuses a handle in BB_ERR_DEVICE / BB_ERR_STATE.  One launch, asynchronous, no
 * allocation, graph-capturable from the first call. */
typedef struct bb_eval_weights {
  bb_greedy_weights base;                /* the eight terms, unchanged */
  int32_t perimeter, room3, room5, fits; /* state terms of the last afterstate's board */
} bb_eval_weights;                       /* twelve int32, 48 bytes */
int bb_plan_actions_ext_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w, int64_t w_stride,
                            int32_t depth, const bb_plan_out* out, void* stream);
int bb_plan_actions_ext(bb_env* env, const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                        const bb_plan_out* out, void* stream);

/* ---- per-action full-hand values and the hand-safe mask -----------------------
 * What bb_plan_actions folds into one maximum, kept per first move.  The search
 * is search(P, depth) above, move for move (engine.py:326-346, 390-431, 348-362;
 * the hand is dealt together, engine.py:155-172, and refilled only after its
 * third piece, engine.py:432-437); the reference has no such call.  For action
 * a of position i, over the maximal sequences whose first move is a:
 *   q      [n][192] the largest value (move terms summed along the sequence +
 *                   state terms of its last afterstate, int64); INT64_MIN when
 *                   a is illegal
 *   rest   [n][192] a_2 | a_3 << 8 of the best such sequence, ties to the
 *                   lexicographically lowest (a_2, a_3); 0xFF stands for a ply
 *                   not played (a sequence that ends at ply 1: 0xFFFF); -1 when
 *                   a is illegal
 *   leaves [n][192] the number of such sequences; 0 when a is illegal
 *   safe   [n][3]   mask word of hand slot p: bit c is set iff action p*64 + c
 *                   is legal and at least one maximal sequence that starts with
 *                   it ends in an afterstate with dead == 0.  The layout is
 *                   that of bb_obs / bb_snapshot mask_bits, so the words go
 *                   straight into bb_random_actions and bb_masked_sample.  safe
 *                   does not depend on w.  At depth 1 it is legal & !dead.  At
 *                   depth 2 and depth 3 it is the same set: a ply-2 afterstate
 *                   that is neither a refill nor dead means the hand was whole
 *                   and its last piece fits, so a third move exists, and that
 *                   move is a refill, which is never dead.
 * With the same w and depth, bb_plan_actions' value is max_a q, its action the
 * lowest a attaining it, its plan[1:] the decoded rest[action] and its leaves
 * the sum of leaves over a.  Any output may be NULL, not all four.  depth is
 * 1..3; n == 0 does nothing.  BB_ERR_ARG (the rule named in bb_last_error,
 * before any HIP call) for a NULL pos / pos->board / pos->hand / w / out, all
 * four outputs NULL, n < 0 and depth outside 1..3.  The handle form reads the
 * live columns and changes nothing, the RNG included, and refuses a handle in
 * BB_ERR_DEVICE / BB_ERR_STATE.  Asynchronous on `stream`, no allocation, no
 * sync (graph-capturable from the first call); indexing is 64-bit. */
typedef struct bb_plan_values_out {
  int64_t*  q;       /* [n][192] */
  int32_t*  rest;    /* [n][192] */
  int32_t*  leaves;  /* [n][192] */
  uint64_t* safe;    /* [n][3]   */
} bb_plan_values_out;   /* device pointers; any may be NULL, not all four */

int bb_plan_values_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t depth,
                       const bb_plan_values_out* out, void* stream);
int bb_plan_values(bb_env* env, const bb_greedy_weights* w, int32_t depth, const bb_plan_values_out* out, void* stream);

/* ---- the hand-safe mask alone --------------------------------------------------
 * bb_plan_values' safe words of depth >= 2 without the values: an existence
 * search, integers only, no weights.  Action a = p*64 + c of position (B, hand)
 * is legal as bb_afterstates defines it (the hand's game-over bit clear, slot p
 * unused, piece id < BB_NUM_PIECES, the piece fits at c).  With
 * B1 = clear_full(B | shape << c), a legal a is safe iff
 *   - it uses the last unused slot (a refill); or
 *   - one slot q stays unused and its piece has an anchor on B1; or
 *   - two slots b, c stay unused and for one of the orders (b, c), (c, b) the
 *     first piece has an anchor x on B1 such that the second piece has an anchor
 *     on clear_full(B1 | first.shape << x).
 * (An unused slot whose piece id is >= BB_NUM_PIECES has no anchor anywhere.)
 * This is not the depth-1 set legal & !dead.
 *   mode BB_SAFE_WORDS    d_mask[i][p] = the safe word of slot p (zeros where
 *                         nothing is safe)
 *   mode BB_SAFE_OR_LEGAL the sampling mask: the safe words where position i has
 *                         a safe action, else its legal words (as computed here)
 * d_mask has the layout of bb_obs / bb_snapshot mask_bits.  pos->combo and
 * pos->prev are not read.  n == 0 does nothing.  BB_ERR_ARG (the rule named in
 * bb_last_error, before any HIP call) for a NULL pos / pos->board / pos->hand /
 * d_mask, n < 0 and a mode outside 0..1.  The handle form reads the live columns
 * and changes nothing, the RNG included, and refuses a handle in BB_ERR_DEVICE /
 * BB_ERR_STATE.  Asynchronous on `stream`, no allocation, no sync
 * (graph-capturable from the first call); indexing is 64-bit. */
#define BB_SAFE_WORDS 0
#define BB_SAFE_OR_LEGAL 1
int bb_safe_mask_pos(const bb_positions* pos, int32_t n, int32_t mode, uint64_t* d_mask /* [n][3] */, void* stream);
int bb_safe_mask(bb_env* env, int32_t mode, uint64_t* d_mask /* [N][3] */, void* stream);

/* ---- the refill census -----------------------------------------------------------
 * Replaces the dealer's acceptance test of engine.py:155-224 (_generate_valid_pieces
 * with _can_place_all_pieces) as a random experiment by its exact outcome space: for
 * a board B, which of the 37^3 ordered hands (a, b, c) the dealer would accept.
 * Integers only.  A hand {a, b, c} is solvable on B iff for some order (x, y, z) of it
 * there are anchors such that x fits B, y fits B1 = clear_full(B | x) and z fits
 * clear_full(B1 | y): _can_place_all_pieces, and the same predicate as "bb_safe_mask
 * mode 0 gives a non-zero word for the whole hand (a, b, c)".  It does not depend on
 * the order, so
 *   solvable[i][a][b]  bit c = hand {a, b, c} is solvable on board i; symmetric under
 *                      every permutation of (a, b, c); bits 37..63 are zero
 *   count[i]           = sum over a, b of popcount(solvable[i][a][b]), 0..BB_NUM_HANDS
 * With p = count / BB_NUM_HANDS the dealer (up to 100 uniform draws, the 100th kept
 * whatever it is) hands out a hand that cannot be played with probability (1 - p)^100.
 * A crafted board with full lines is taken as it is, as in bb_afterstates.  Only the
 * board is read: no hand, combo or reward config.  n == 0 does nothing.  BB_ERR_ARG
 * (the rule named in bb_last_error, before any HIP call) for a NULL board, n < 0, a
 * NULL out and an out with both pointers NULL.  The handle form reads the live board
 * column and changes nothing, the RNG included, and refuses a handle in
 * BB_ERR_DEVICE / BB_ERR_STATE.  Asynchronous on `stream`, no allocation, no sync
 * (graph-capturable from the first call); indexing is 64-bit. */
#define BB_NUM_HANDS 50653            /* 37^3 ordered hands */
typedef struct bb_census_out {
  int32_t*  count;     /* [n]          ordered hands (a,b,c) that engine.py:174-224 accepts on the board, 0..50653 */
  uint64_t* solvable;  /* [n][37][37]  bit c of word [a][b] = hand {a,b,c} can be placed in some order; symmetric
                          under every permutation of (a,b,c); bits 37..63 are zero */
} bb_census_out;       /* device pointers (host pointers for libbbvec_host.so); either may be NULL, not both */
/* replaces engine.py:155-224 for the positions given as a board column */
int bb_refill_census_pos(const uint64_t* d_board, int32_t n, const bb_census_out* out, void* stream);
/* replaces engine.py:155-224 for the handle's live boards ([N] / [N][37][37] outputs) */
int bb_refill_census(bb_env* env, const bb_census_out* out, void* stream);

/* ---- dealt next-hand values (the chance node behind a refill) ----------------------
 * Replaces engine.py:155-172 (_generate_valid_pieces: up to 100 uniform draws of three
 * pieces, the first hand that _can_place_all_pieces accepts, else the 100th) for a
 * board that is not a live env, with a counter-based generator in place of the env's
 * PCG64 stream, and searches every dealt hand.  Integers only.  For board i and deal
 * j < deals, draw t = 0..99 takes the four Philox4x32-10 words of counter
 *   (idx, step) = (d_stream ? d_stream[i] : i, (uint64)j << 7 | t)  under key `seed`
 * (bb_random_actions' generator: c0,c1 = idx lo,hi; c2,c3 = step lo,hi; k0,k1 = seed
 * lo,hi) and makes the piece ids (word_k * 37) >> 32 for k = 0, 1, 2; word 3 is not
 * used.  Bias: 2^32 = 37 * 116,080,197 + 7, so seven of the 37 ids have 116,080,198
 * words each and thirty have 116,080,197 -- a relative excess of 8.6e-9, against the
 * reference's exactly uniform Lemire draw.  The first draw whose hand is solvable on
 * the board (the predicate of bb_refill_census: some order and anchors place all
 * three, with the line clears in between) is kept; after 100 refusals the 100th is.
 * Two boards given the same stream id and seed meet the same draws (common random
 * numbers) and differ only where their acceptance differs.
 *   hand     [n][deals] the dealt hand word a | b << 6 | c << 12: nothing used, not
 *                       over, has_uint32 0
 *   value    [n][deals] what bb_plan_actions_pos returns as `value` for the position
 *                       (board i, that hand, combo[i]) under w and depth; a hand
 *                       without a legal first move (INT64_MIN there) gets (int64)w.dead
 *   attempts [n][deals] k in 1..100: the k-th draw was accepted; -100: all refused
 * d_combo NULL reads as 0.  depth is 1..3, deals 1..BB_REFILL_MAX_DEALS; n == 0 does
 * nothing.  BB_ERR_ARG (the rule named in bb_last_error, before any HIP call) for a
 * NULL board, n < 0, a NULL w, a NULL out, all three outputs NULL, depth outside 1..3
 * and deals outside 1..1024.  The handle form reads the live board and combo columns
 * and changes nothing, the RNG included, and refuses a handle in BB_ERR_DEVICE /
 * BB_ERR_STATE.  Asynchronous on `stream`, no allocation, no sync (graph-capturable
 * from the first call); indexing is 64-bit. */
#define BB_REFILL_MAX_DEALS 1024
typedef struct bb_refill_values_out {
  uint32_t* hand;      /* [n][m] the dealt hand word: ids a | b<<6 | c<<12, nothing used, not over, has_uint32 0 */
  int64_t*  value;     /* [n][m] best full-hand value of that hand on the board (above)                          */
  int32_t*  attempts;  /* [n][m] k in 1..100: the k-th draw was accepted; -100: all refused, the 100th is kept    */
} bb_refill_values_out;  /* device pointers (host pointers for libbbvec_host.so); any may be NULL, not all three */
/* replaces engine.py:155-172 for boards given as columns, and searches the hands */
int bb_refill_values_pos(const uint64_t* d_board, const int32_t* d_combo /* NULL = 0 */,
                         const uint64_t* d_stream /* NULL = i */, int32_t n, const bb_greedy_weights* w,
                         int32_t depth, int32_t deals /* m */, uint64_t seed,
                         const bb_refill_values_out* out, void* stream);
/* the same for the handle's live boards and combos ([N][m] outputs) */
int bb_refill_values(bb_env* env, const uint64_t* d_stream, const bb_greedy_weights* w, int32_t depth,
                     int32_t deals, uint64_t seed, const bb_refill_values_out* out, void* stream);

/* ---- per-action values and dealt next-hand values with the shape terms ---------------
 * bb_plan_values and bb_refill_values under rows of bb_eval_weights, as bb_plan_actions_ext
 * is to bb_plan_actions.  d_w are rows of twelve int32 in the struct's field order, in the
 * memory of the position columns (device memory for libbbvec.so, host memory for
 * libbbvec_host.so), read when the launch runs.  w_stride 0: every position (board) uses
 * d_w[0]; 1: position (board) i uses d_w[i]; any other value is refused.
 *
 * bb_plan_values_ext: q, rest, leaves and safe as bb_plan_values defines them, with the
 * value of a maximal sequence gaining
 *   w.perimeter*perimeter(B_k) + w.room3*room3(B_k) + w.room5*room5(B_k) + w.fits*fits(B_k)
 * for B_k the board of its last afterstate after the clears, at dead and refill leaves
 * alike, a sequence that ends at ply 1 included.  safe and leaves do not depend on the
 * row.  With the same row and depth, bb_plan_actions_ext's value is max_a q, its action
 * the lowest a attaining it, its plan[1:] the decoded rest[action] and its leaves the sum
 * of leaves over a.
 *
 * bb_refill_values_ext: hand and attempts are bit for bit bb_refill_values' (the deal reads
 * no weights); every deal of board i is searched under board i's row, and value is what
 * bb_plan_actions_ext_pos returns for (board i, that hand, combo[i]).  A dealt hand with no
 * legal first move gets (int64)w.base.dead and nothing else: there is no afterstate whose
 * board the terms could read.
 *
 * With the four shape weights 0 in a row the answers for that position (board) are those
 * of bb_plan_values(_pos) / bb_refill_values(_pos) under `base`.  Refusals (BB_ERR_ARG, the
 * rule named in bb_last_error, before any HIP call) are those of bb_plan_values /
 * bb_refill_values with "weight rows" for "weights", plus a w_stride that is not 0 or 1;
 * n == 0 does nothing.  The handle forms read the live columns, change nothing, the RNG
 * included, and refuse a handle in BB_ERR_DEVICE / BB_ERR_STATE.  One launch, integers
 * only, asynchronous, no allocation, no sync (graph-capturable from the first call);
 * indexing is 64-bit. */
int bb_plan_values_ext_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w, int64_t w_stride,
                           int32_t depth, const bb_plan_values_out* out, void* stream);
int bb_plan_values_ext(bb_env* env, const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                       const bb_plan_values_out* out, void* stream);
int bb_refill_values_ext_pos(const uint64_t* d_board, const int32_t* d_combo, const uint64_t* d_stream, int32_t n,
                             const bb_eval_weights* d_w, int64_t w_stride, int32_t depth, int32_t deals,
                             uint64_t seed, const bb_refill_values_out* out, void* stream);
int bb_refill_values_ext(bb_env* env, const uint64_t* d_stream, const bb_eval_weights* d_w, int64_t w_stride,
                         int32_t depth, int32_t deals, uint64_t seed, const bb_refill_values_out* out, void* stream);

/* ---- a plan played to its leaf ------------------------------------------------------
 * Plays d_plan[i][0..2] from position i with the one-ply move of bb_afterstates
 * (engine.py:326-346 legality, 390-431 place / clear / combo / score).  A plan entry
 * is an action 0..191, or negative for a ply not played (as bb_plan_out.plan and the
 * decoded rest of bb_plan_values give them): play ends at the first negative entry.
 * An entry that is not a legal action of the position reached (>= 192 included) sets
 * status bit 4 and play stops before it; the outputs describe the state reached.
 *   board, hand, combo [n]  after the last ply played (hand: the slots played marked
 *                           used, the other bits as they came); the inputs when none
 *   lines  [n]  lines cleared, summed over the plies played
 *   score  [n]  score_gained, summed over the plies played (combo carried)
 *   status [n]  bits 0-1 plies played (0..3) | bit 2 the last afterstate is dead (no
 *               unused slot fits, not a refill) | bit 3 it is a refill (all three slots
 *               used) | bit 4 a ply was illegal
 * pos->combo NULL reads as 0; pos->prev is not read.  Any output may be NULL, not all
 * six; n == 0 does nothing.  BB_ERR_ARG (the rule named in bb_last_error, before any
 * HIP call) for NULL positions, n < 0, a NULL d_plan, a NULL out and all outputs NULL.
 * Asynchronous on `stream`, no allocation, no sync (graph-capturable from the first
 * call); indexing is 64-bit. */
#define BB_PLAY_PLIES 3u     /* status & BB_PLAY_PLIES: plies played */
#define BB_PLAY_DEAD 4u
#define BB_PLAY_REFILL 8u
#define BB_PLAY_ILLEGAL 16u
typedef struct bb_play_plan_out {
  uint64_t* board;   /* [n] */
  uint32_t* hand;    /* [n] */
  int32_t*  combo;   /* [n] */
  int32_t*  lines;   /* [n] */
  int64_t*  score;   /* [n] */
  int32_t*  status;  /* [n] */
} bb_play_plan_out;  /* device pointers (host pointers for libbbvec_host.so); any may be NULL, not all six */
int bb_play_plan_pos(const bb_positions* pos, int32_t n, const int32_t* d_plan /* [n][3] */,
                     const bb_play_plan_out* out, void* stream);

/* ---- the two-hand decision: one chance node behind the hand, in one call ---------------
 * The search past the refill that agents/greedy.py TwoHandPlanAgent._decide composes from
 * bb_plan_values_ext, a sort, bb_play_plan_pos and bb_refill_values_ext, with no host read
 * in between.  Integers only; every output is defined over those entry points.  For
 * position i with row w = d_w[i * w_stride] (rows as bb_plan_values_ext takes them):
 *   1. q, rest = bb_plan_values_ext_pos under w and depth.
 *   2. The candidates are the K actions with the largest q, ties to the lower action (a
 *      stable descending sort); an action with q == INT64_MIN is never one, so fewer
 *      legal actions give fewer candidates.
 *   3. Candidate a's leaf is bb_play_plan_pos on (a, decoded rest[a]) from
 *      (board, hand, combo).
 *   4. A leaf with BB_PLAY_REFILL set gets
 *        Q2[a] = deals * (w.base.lines * lines + w.base.score * score) + sum_j value_j
 *      with value_j what bb_refill_values_ext_pos gives for (leaf board, leaf combo, stream
 *      id d_stream ? d_stream[i] : i, seed, deal j) under the ROOT's row w.  All candidates
 *      of a root share one stream id and so meet the same draws; two roots with the same
 *      stream id share theirs.
 *   5. Any other leaf (dead, or cut short by depth) keeps Q2[a] = deals * q[a].
 *   6. action is the lowest action with the largest Q2, 0 when there is no candidate.
 * Outputs:
 *   action [n]            the decision
 *   q2     [n][192]       Q2 of the candidates; INT64_MIN for every other action
 *   cand   [n][K]         the candidates in rank order; -1 for an absent one
 *   status [n][K]         bb_play_plan_pos' status word of the candidate's leaf; -1 if absent
 *   value  [n][K][deals]  the dealt hands' values; 0 where no deal was made (absent
 *                         candidate, or a leaf that is no refill)
 * With the four shape weights of a row 0 the answers are those of the eight-weight calls
 * under `base`.  d_work is caller-owned scratch of at least bb_plan2_work_bytes(n, K, deals)
 * bytes, 8-byte aligned, in the memory of the position columns; its contents after the call
 * are unspecified and the call allocates nothing.  bb_plan2_work_bytes is a host-side size
 * query, negative for n < 0, candidates outside 1..192 or deals outside
 * 1..BB_REFILL_MAX_DEALS.  n == 0 does nothing.  BB_ERR_ARG (the rule named in
 * bb_last_error, before any HIP call) for NULL positions, n < 0, NULL rows, a w_stride that
 * is not 0 or 1, a NULL out, all five outputs NULL, depth outside 1..3, candidates outside
 * 1..192, deals outside 1..1024, a NULL d_work and work_bytes below the size query.  The
 * handle form reads the live board, hand and combo columns (n is the handle's env count),
 * changes nothing, the RNG included, and refuses a handle in BB_ERR_DEVICE / BB_ERR_STATE.
 * Four launches on `stream`, asynchronous, no sync, no host read, 64-bit indexing,
 * graph-capturable from the first call.  seed is passed by value: a captured graph replays
 * the seed it was captured with, so every replay repeats its deals. */
int64_t bb_plan2_work_bytes(int32_t n, int32_t candidates, int32_t deals);
typedef struct bb_plan2_out {
  int32_t* action;  /* [n]            the decision; 0 when the position has no legal action            */
  int64_t* q2;      /* [n][192]       Q2 of the candidates; INT64_MIN for every other action           */
  int32_t* cand;    /* [n][K]         the candidates in rank order; -1 for an absent one               */
  int32_t* status;  /* [n][K]         bb_play_plan's status word of the candidate's leaf; -1 if absent */
  int64_t* value;   /* [n][K][deals]  the dealt hands' values; 0 where no deal was made                */
} bb_plan2_out;     /* device pointers (host pointers for libbbvec_host.so); any may be NULL, not all five */
int bb_plan2_values_pos(const bb_positions* pos, const uint64_t* d_stream /* NULL = i */, int32_t n,
                        const bb_eval_weights* d_w, int64_t w_stride, int32_t depth, int32_t candidates /* K */,
                        int32_t deals, uint64_t seed, void* d_work, int64_t work_bytes, const bb_plan2_out* out,
                        void* stream);
int bb_plan2_values(bb_env* env, const uint64_t* d_stream, const bb_eval_weights* d_w, int64_t w_stride,
                    int32_t depth, int32_t candidates, int32_t deals, uint64_t seed, void* d_work,
                    int64_t work_bytes, const bb_plan2_out* out, void* stream);

/* ---- dealt playouts: several hands past the refill, in one launch -------------------------
 * The plan agent played for `hands` hands under a counter-based dealer: deal, search, play the
 * plan found, deal again.  Integers only; every output is defined over bb_refill_values_ext,
 * bb_plan_actions_ext_pos and bb_play_plan_pos.  Rows, w_stride, d_combo and d_stream as
 * bb_refill_values_ext(_pos) takes them; every playout of board i runs under board i's row
 * d_w[i * w_stride] and stream id idx = d_stream ? d_stream[i] : i.  For board i and playout
 * j < playouts:
 *   1. (B, combo) = (board[i], combo[i]), moved = 0.
 *   2. For h = 0 .. hands-1:
 *      deal    the hand that bb_refill_values' law deals as deal j on B under stream id idx
 *              and key (seed + h) mod 2^64: the same counters, the same 100 draws, the same
 *              acceptance.  Hand 0 is bit for bit bb_refill_values_ext's deal j.
 *      search  value_h, plan_h = bb_plan_actions_ext_pos on (B, that hand, combo) under the
 *              row and depth.  No legal first move: value_h = (int64)w.base.dead, nothing is
 *              played, and the playout ends with status 0.
 *      play    plan_h as bb_play_plan_pos plays it, the combo carried: B, combo, lines, score
 *              and plies advance; m_h = w.base.lines * lines_h + w.base.score * score_h.
 *      go on   if that call's status word has BB_PLAY_REFILL and h < hands-1, moved += m_h and
 *              the next hand is dealt; otherwise the playout stops (a dead leaf, a plan cut
 *              short by depth < 3, the last hand).
 *   3. Outputs, each [n][playouts]:
 *      value   moved + value_last: the move terms of every earlier hand plus the last search's
 *              value.  With hands == 1 this is bb_refill_values_ext's value.
 *      score, lines, plies  summed over every ply played
 *      hands   hands searched, 1..hands
 *      status  the last hand's bb_play_plan_pos status word, 0 if it had no legal first move;
 *              BB_PLAY_REFILL set: the playout survived all `hands` hands
 *      board, combo  after the last ply played
 *      hand    the last hand dealt, in bb_refill_values_out.hand's format
 * Two playouts with the same stream id and j meet the same draws (common random numbers).
 * Started from empty boards with one row per board this plays whole games of the plan agent.
 * depth is 1..3, playouts 1..1024, hands 1..BB_PLAYOUT_MAX_HANDS; n == 0 does nothing.
 * BB_ERR_ARG (the rule named in bb_last_error, before any HIP call) for a NULL board, n < 0,
 * NULL rows, a w_stride that is not 0 or 1, a NULL out, all nine outputs NULL, depth outside
 * 1..3, playouts outside 1..1024 and hands outside 1..256.  The handle form reads the live
 * board and combo columns and changes nothing, the RNG included, and refuses a handle in
 * BB_ERR_DEVICE / BB_ERR_STATE.  One launch, asynchronous on `stream`, no allocation, no sync,
 * no host read (graph-capturable from the first call; seed is passed by value, so a captured
 * graph repeats its deals); indexing is 64-bit. */
#define BB_PLAYOUT_MAX_HANDS 256
typedef struct bb_playout_out {
  int64_t*  value;   /* [n][playouts] moved + the last search's value                              */
  int64_t*  score;   /* [n][playouts] score_gained over every ply played (combo carried)           */
  int32_t*  lines;   /* [n][playouts] lines cleared over every ply played                          */
  int32_t*  plies;   /* [n][playouts] plies played                                                 */
  int32_t*  hands;   /* [n][playouts] hands searched, 1..hands                                     */
  int32_t*  status;  /* [n][playouts] the last hand's play-plan status word; 0: no legal first move */
  uint64_t* board;   /* [n][playouts] after the last ply played                                    */
  int32_t*  combo;   /* [n][playouts] after the last ply played                                    */
  uint32_t* hand;    /* [n][playouts] the last hand dealt: ids a | b<<6 | c<<12                    */
} bb_playout_out;    /* device pointers (host pointers for libbbvec_host.so); any may be NULL, not all nine */
int bb_playout_values_pos(const uint64_t* d_board, const int32_t* d_combo /* NULL = 0 */,
                          const uint64_t* d_stream /* NULL = i */, int32_t n, const bb_eval_weights* d_w,
                          int64_t w_stride, int32_t depth, int32_t playouts, int32_t hands, uint64_t seed,
                          const bb_playout_out* out, void* stream);
/* the same for the handle's live boards and combos ([N][playouts] outputs) */
int bb_playout_values(bb_env* env, const uint64_t* d_stream, const bb_eval_weights* d_w, int64_t w_stride,
                      int32_t depth, int32_t playouts, int32_t hands, uint64_t seed, const bb_playout_out* out,
                      void* stream);

/* Fused masked-categorical tail of BlockBlastNetwork.get_action_and_value
 * (network.py:173-180, 210-262; Categorical clamp semantics of torch 2.10):
 * logits f32 [n][192] (raw policy-head output, unmasked) + mask bits ->
 *   action (inverse-CDF sample with u from d_uniform[i] if non-NULL, else from
 *   Philox(seed, (env_offset+i, step)) word 1; argmax when deterministic),
 *   logp = log(clamp(p_a, 2^-23, 1-2^-23)), entropy = masked renormalised
 *   entropy with 1e-10 clamps.  Any of action/logp/entropy may be NULL.
 *   If d_action_in is non-NULL it is evaluated instead of sampling. */
int bb_masked_sample(const float* d_logits, const uint64_t* d_mask_bits,
                     int32_t n, const float* d_uniform, uint64_t seed,
                     uint64_t step, uint64_t env_offset, int32_t deterministic,
                     const int64_t* d_action_in, int64_t* d_action,
                     float* d_logp, float* d_entropy, void* stream);

/* bb_masked_sample with the Philox step read from device memory:
 * step = *d_step + step_add (no d_uniform, no d_action_in).  For a rollout
 * captured in a HIP graph (scripts/train.py:173-203 replayed per update):
 * the captured launches keep their step_add (0 .. T-1) and the caller
 * advances *d_step by T between replays, so every replay samples with fresh
 * uniforms, exactly as T eager calls with step = base + t would. */
int bb_masked_sample_dstep(const float* d_logits, const uint64_t* d_mask_bits,
                           int32_t n, uint64_t seed, const uint64_t* d_step,
                           uint64_t step_add, uint64_t env_offset,
                           int32_t deterministic, int64_t* d_action,
                           float* d_logp, float* d_entropy, void* stream);

/* GAE (RolloutBuffer.compute_returns_and_advantages, ppo.py:141-169) over
 * [T][N] f32 arrays, numpy-2 float32 operation order, no FMA contraction.
 * gamma and gamma_lambda are the f32 roundings of gamma and gamma*gae_lambda
 * (the latter multiplied in double first, as Python does). */
int bb_gae(const float* d_rewards, const float* d_values, const float* d_dones,
           const float* d_last_values, int32_t T, int32_t N, float gamma,
           float gamma_lambda, float* d_adv, float* d_ret, void* stream);

/* Packed rollout-buffer record -> network input for a minibatch
 * (RolloutBuffer.get_samples, ppo.py:171-213, with obs kept packed on device):
 * for j < n, src = d_index[j]: x[j] = expand(board[src], hand[src]),
 * mask_f32[j] = bits(mask[src]).  Either output may be NULL. */
int bb_gather_obs(const uint64_t* d_board, const uint32_t* d_hand,
                  const uint64_t* d_mask_bits, const int64_t* d_index,
                  int32_t n, float* d_x, float* d_mask_f32, void* stream);

/* Training-mode BatchNorm2d with an optional fused ReLU and an optional fused
 * bias of the preceding convolution, for the policy/value CNN's conv stack
 * (network.py:75-117 conv -> BatchNorm2d -> ReLU, ResidualBlock
 * network.py:14-30).  Input x is the convolution output WITHOUT its bias;
 * pre_bias (NULL = none) is that bias, added per channel before the
 * statistics, so the result equals nn.BatchNorm2d(conv(x) + bias).
 * dtype 0 = f32, 1 = bf16 activations; nhwc 0 = NCHW contiguous (HW * element
 * size a multiple of 16 bytes), 1 = NHWC / channels_last contiguous (C *
 * element size = 16 bytes times a power of two <= 256); weight / bias /
 * statistics are f32.  Forward = nn.BatchNorm2d training forward (batch mean,
 * biased variance for the normalisation; running_mean / running_var updated
 * with `momentum` and the unbiased variance when non-NULL, num_batches_tracked
 * incremented when non-NULL), then max(y, 0) if relu.  ws is caller scratch of
 * bb_bn_workspace_bytes(...) bytes (16-byte aligned).  Backward takes the
 * forward's input x and saved mean / inverse std; with relu it recomputes the
 * mask from x.  It writes dx and, where non-NULL, dweight, dbias and
 * dpre_bias = sum of dx per channel.  Three launches each (two with `part`).
 * No atomics: results are deterministic.  All pointers are device pointers;
 * every optional field is "NULL / 0: absent".
 * Shape rule, checked by all three entry points: an NCHW row (HW elements) is
 * at most 256 16-byte vectors, so HW <= 1024 for f32 and HW <= 2048 for bf16;
 * bb_bn_workspace_bytes returns -1 and the launches BB_ERR_ARG for any shape,
 * dtype or layout outside the rules above. */
int64_t bb_bn_workspace_bytes(int32_t dtype, int32_t nhwc, int32_t N, int32_t C, int32_t HW);

typedef struct bb_bn_fwd {
  const void* x;            /* [N][C][HW] or [N][HW][C], required                               */
  const void* res;          /* optional residual (ResidualBlock, network.py:14-30: relu(bn2(conv2(.)) + x)),
                               x's shape, dtype and layout, 16-byte aligned: y = [relu](round(BatchNorm(x +
                               pre_bias)) + res), round = the activation dtype's rounding (the BatchNorm output
                               tensor of the unfused module), the sum rounded once, as torch's add */
  int32_t dtype, nhwc, N, C, HW;
  const float* pre_bias;    /* [C] optional                                                     */
  const float* weight;      /* [C] required                                                     */
  const float* bias;        /* [C] required                                                     */
  float eps;
  int32_t relu;
  double* ws;               /* required                                                         */
  float* save_mean;         /* [C] required                                                     */
  float* save_invstd;       /* [C] required                                                     */
  float* running_mean;      /* [C] optional                                                     */
  float* running_var;       /* [C] optional                                                     */
  float momentum;
  int64_t* num_batches_tracked; /* optional                                                     */
  void* y;                  /* x's shape, required                                              */
  const double* part;       /* optional: statistics partials [nb_part][C][3] a board convolution's forward already
                               produced (bb_conv3x3_forward_stats, nb_part = bb_conv3x3_stats_blocks(N, C))
                               instead of a reduction pass over x                               */
  int32_t nb_part;          /* > 0 with part                                                    */
} bb_bn_fwd;

/* A board convolution's pending weight-gradient reduction (bb_conv3x3_wgrad_reduce's arguments), run as extra
 * workgroups of a BatchNorm backward's finalisation launch: two small launches in one.  ws NULL: no job. */
typedef struct bb_wgrad_reduce {
  const float* ws;
  int32_t chunks, cin, cout, w_layout;
  float* dw;
} bb_wgrad_reduce;

typedef struct bb_bn_bwd {
  const void* x;            /* the forward's input, required                                    */
  const void* dy;           /* x's shape, required                                              */
  const void* y;            /* optional, with gres: the forward's output, whose ReLU (after a residual add) is
                               undone here: the backward runs over g = (y > 0 ? dy : 0) (torch's
                               threshold_backward), which the reduction pass writes to gres and the elementwise
                               pass reads; g is also the residual's gradient.  relu must be 0; not with part */
  int32_t dtype, nhwc, N, C, HW;
  const float* pre_bias;    /* [C] optional                                                     */
  const float* weight;      /* [C] required                                                     */
  const float* bias;        /* [C] required                                                     */
  const float* save_mean;   /* [C] required                                                     */
  const float* save_invstd; /* [C] required                                                     */
  int32_t relu;
  double* ws;               /* required                                                         */
  void* dx;                 /* x's shape, required                                              */
  float* dweight;           /* [C] optional                                                     */
  float* dbias;             /* [C] optional                                                     */
  float* dpre_bias;         /* [C] optional                                                     */
  void* gres;               /* x's shape; required with y, absent without                       */
  bb_wgrad_reduce reduce;   /* optional (reduce.ws NULL: none)                                  */
  const double* part;       /* optional: reduction partials [nb_part][C][3] the board convolution that produced dy
                               already made (bb_conv3x3_forward_bstats) instead of a pass over x and dy */
  int32_t nb_part;          /* > 0 with part                                                    */
} bb_bn_bwd;

int bb_bn_forward(const bb_bn_fwd* a, void* stream);
int bb_bn_backward(const bb_bn_bwd* a, void* stream);

/* The PPO minibatch loss (PPOAgent.update, ppo.py:362-401) with the masked
 * Categorical tail (network.py:173-180, 210-262), fused, forward and backward.
 * Per row i < B: logits [B][192] (raw policy head), mask f32 [B][192]
 * (non-zero = legal), action, old log-prob, advantage, return and value.
 * logits / values and their gradients are f32 (bf16 = 0) or bf16 (1: the
 * autocast network's outputs, widened exactly on load; the gradients rounded
 * to nearest even: exactly the values of autograd's casts around the f32 loss,
 * bit-identical, without the four cast launches).
 * Forward writes stats[6] = {policy_loss, value_loss, entropy, total_loss,
 * approx_kl, clip_fraction} (the reference's update metrics) and, if non-NULL,
 * loss[0] = total_loss, in one launch: ws is scratch of
 * bb_ppo_loss_workspace_bytes(B) bytes for the blocks' partial sums, which the
 * last block to finish adds in a fixed order (deterministic); cnt is one
 * uint32 counter, zero before the first launch and re-armed by each (one
 * counter per stream).  Backward takes d(total_loss) from grad_loss[0]
 * (device memory, so a HIP graph can replay it) and writes dlogits [B][192]
 * and dvalues [B], following torch autograd's rules for min / clamp / log.
 * bb_ppo_loss_fused is both in one launch (the caller knows the loss gradient
 * before the forward: the root of its backward). */
int64_t bb_ppo_loss_workspace_bytes(int32_t B);

typedef struct bb_ppo_loss_args {
  const void* logits;       /* [B][192]                                  all: required */
  const void* values;       /* [B]                                                     */
  int32_t bf16;
  const float* mask;        /* [B][192]                                                */
  const int64_t* actions;   /* [B]                                                     */
  const float* old_logp;    /* [B]                                                     */
  const float* adv;         /* [B]                                                     */
  const float* ret;         /* [B]                                                     */
  int32_t B;
  float clip, value_coef, entropy_coef;
  const float* grad_loss;   /* [1]       backward, fused: required; forward: unused    */
  void* dlogits;            /* [B][192]  backward, fused: required; forward: unused    */
  void* dvalues;            /* [B]       backward, fused: required; forward: unused    */
  double* ws;               /*           forward, fused: required; backward: unused    */
  uint32_t* cnt;            /* [1]       forward, fused: required; backward: unused    */
  float* stats;             /* [6]       forward, fused: required; backward: unused    */
  float* loss;              /* [1]       forward, fused: optional; backward: unused    */
} bb_ppo_loss_args;

int bb_ppo_loss_forward(const bb_ppo_loss_args* a, void* stream);
int bb_ppo_loss_backward(const bb_ppo_loss_args* a, void* stream);
int bb_ppo_loss_fused(const bb_ppo_loss_args* a, void* stream);

/* Policy distillation from the full-hand search: the cross-entropy between a
 * softmax over bb_plan_values' per-action values and the masked policy, fused,
 * forward and backward.  Per row i < B: logits [B][192] (raw policy head; f32,
 * or bf16 widened exactly on load, as bb_ppo_loss_args.bf16), mask_bits [B][3]
 * (layout of bb_obs / bb_snapshot mask_bits: the words the policy samples
 * under) and q [B][192] (exactly what bb_plan_values writes, INT64_MIN =
 * illegal).  With M the actions whose mask bit is set, S the a in M with
 * q[a] != INT64_MIN and qmax the maximum of q over S:
 *   target   tau > 0: t[a] = exp(float(q[a] - qmax) / tau) / Z over S (the
 *            difference in int64, exact; below -2^31: t[a] = 0);
 *            tau == 0: one-hot on the lowest a attaining qmax (bb_plan_actions'
 *            action)
 *   student  logpi = log_softmax(logits + where(M, 0, -inf)) by max-subtraction,
 *            no clamp; pi = exp(logpi)
 *   ce_i = -sum_{t[a] > 0} t[a] logpi[a]   ht_i = -sum t log t
 *   hp_i = -sum_M pi log pi
 *   agree_i = 1 when the lowest-index argmax of the logits over M is the
 *            lowest-index argmax of q over S
 * A row with empty S (a finished game, a stale mask) adds 0 to every sum and
 * all of its gradients are 0.  Forward writes stats[6] = {cross_entropy, kl,
 * target_entropy, policy_entropy, agreement, rows}: the first five are sums
 * over rows divided by B, kl = cross_entropy - target_entropy, rows counts the
 * rows with non-empty S; and, if non-NULL, loss[0] = cross_entropy.  ws, cnt
 * and the fixed-order sum of fp64 block partials are those of bb_ppo_loss_*
 * (ws of bb_distill_loss_workspace_bytes(B) bytes; cnt one uint32, zero before
 * the first launch, re-armed by each), so two launches are bit-identical.
 * Backward: dlogits[i][a] = grad_loss[0] / B * (pi[a] - t[a]) for a in M, 0
 * outside M and in every entry of an empty-S row; f32, or bf16 rounded to
 * nearest even.  bb_distill_loss_fused is both in one launch and equals them
 * bit for bit.  Asynchronous on the stream, no allocation, graph-capturable
 * from the first call.  B == 0 does nothing. */
int64_t bb_distill_loss_workspace_bytes(int32_t B);

typedef struct bb_distill_loss_args {
  const void* logits;        /* [B][192]                                  all: required */
  int32_t bf16;
  const uint64_t* mask_bits; /* [B][3]                                                  */
  const int64_t* q;          /* [B][192]                                                */
  int32_t B;                 /* >= 0                                                    */
  float tau;                 /* >= 0, finite; in the units of q                         */
  const float* grad_loss;    /* [1]       backward, fused: required; forward: unused    */
  void* dlogits;             /* [B][192]  backward, fused: required; forward: unused    */
  double* ws;                /*           forward, fused: required; backward: unused    */
  uint32_t* cnt;             /* [1]       forward, fused: required; backward: unused    */
  float* stats;              /* [6]       forward, fused: required; backward: unused    */
  float* loss;               /* [1]       forward, fused: optional; backward: unused    */
} bb_distill_loss_args;

int bb_distill_loss_forward(const bb_distill_loss_args* a, void* stream);
int bb_distill_loss_backward(const bb_distill_loss_args* a, void* stream);
int bb_distill_loss_fused(const bb_distill_loss_args* a, void* stream);

/* Search-guided PPO: the PPO minibatch loss and the distillation cross-entropy
 * above on one masked softmax, fused, forward and backward:
 *   total = policy_coef * policy_loss + value_coef * value_loss
 *           - entropy_coef * entropy + distill_coef * cross_entropy
 * With policy_coef = 0 it is distillation that also fits the critic on the
 * rollout's returns; with policy_coef = 1 and a decaying distill_coef it is PPO
 * regularised towards the search.  Per row i < B: logits [B][192] and values
 * [B] (f32, or bf16 as bb_ppo_loss_args.bf16), mask_bits [B][3] (the words the
 * policy sampled under; no f32 mask is read), action, old log-prob, advantage,
 * return, and q [B][192] (exactly what bb_plan_values writes).  With M the
 * actions whose mask bit is set:
 *   PPO half      bb_ppo_loss_*'s row with the mask taken as M: the softmax, the
 *                 p / sum p normalisation, the log-prob clamp at f32 eps, the
 *                 masked entropy with its 1e-10 clamps, the ratio, the clipped
 *                 surrogate, (value - ret)^2, approx_kl and clip_fraction
 *   distillation  bb_distill_loss_*'s row: S, qmax and the int64 difference, the
 *                 -2^31 cut-off, tau == 0 the one-hot of the lowest argmax; ce,
 *                 ht, hp, agree and rows.  A row with empty S adds nothing to
 *                 these five sums and gets no distillation gradient.
 * The row maximum and the sum of exponentials are computed once for both.  A
 * row with empty M adds 0 to every sum and all of its gradients, dvalues
 * included, are 0.  Forward writes stats[12] = {policy_loss, value_loss,
 * entropy, total_loss, approx_kl, clip_fraction, cross_entropy, kl,
 * target_entropy, policy_entropy, agreement, rows}, every mean over B as in the
 * two kernels, and, if non-NULL, loss[0] = total_loss.  With q == NULL the
 * distillation half is skipped and the last six statistics are 0.  ws
 * (bb_guided_loss_workspace_bytes(B) bytes), cnt and the fixed-order sum of
 * fp64 block partials are those of bb_distill_loss_*: two launches are
 * bit-identical.  Backward, with g = grad_loss[0]:
 *   dlogits = g (policy_coef dpolicy - entropy_coef dentropy), by bb_ppo_loss's
 *             formulas (autograd's rules for min / clamp / log), plus
 *             g distill_coef / B (pi - t) on M for rows with non-empty S; 0
 *             outside M
 *   dvalues = g value_coef 2 (value - ret) / B
 * f32, or bf16 rounded to nearest even.  bb_guided_loss_fused is both in one
 * launch and equals them bit for bit.  coefs_dev, when non-NULL, is device
 * memory [5] = {policy_coef, value_coef, entropy_coef, distill_coef, tau} read
 * by the kernel instead of the five scalars, so a captured launch can be
 * replayed under a schedule; its values are the caller's contract.  BB_ERR_ARG,
 * the rule named in bb_last_error, before any HIP call: a NULL struct or
 * required field, B < 0, a negative or non-finite tau, clip or coefficient,
 * q == NULL with distill_coef != 0 or with coefs_dev.  Asynchronous on the
 * stream, no allocation, graph-capturable from the first call.  B == 0 does
 * nothing. */
int64_t bb_guided_loss_workspace_bytes(int32_t B);

typedef struct bb_guided_loss_args {
  const void* logits;        /* [B][192]                                  required      */
  const void* values;        /* [B]                                       required      */
  int32_t bf16;
  const uint64_t* mask_bits; /* [B][3]                                    required      */
  const int64_t* actions;    /* [B]                                       required      */
  const float* old_logp;     /* [B]                                       required      */
  const float* adv;          /* [B]                                       required      */
  const float* ret;          /* [B]                                       required      */
  const int64_t* q;          /* [B][192]  may be NULL iff distill_coef == 0 and coefs_dev == NULL */
  int32_t B;                 /* >= 0                                                    */
  float clip, policy_coef, value_coef, entropy_coef, distill_coef; /* >= 0, finite     */
  float tau;                 /* >= 0, finite; in the units of q                         */
  const float* coefs_dev;    /* [5]       optional: overrides the five scalars after clip */
  const float* grad_loss;    /* [1]       backward, fused: required; forward: unused    */
  void* dlogits;             /* [B][192]  backward, fused: required; forward: unused    */
  void* dvalues;             /* [B]       backward, fused: required; forward: unused    */
  double* ws;                /*           forward, fused: required; backward: unused    */
  uint32_t* cnt;             /* [1]       forward, fused: required; backward: unused    */
  float* stats;              /* [12]      forward, fused: required; backward: unused    */
  float* loss;               /* [1]       forward, fused: optional; backward: unused    */
} bb_guided_loss_args;

int bb_guided_loss_forward(const bb_guided_loss_args* a, void* stream);
int bb_guided_loss_backward(const bb_guided_loss_args* a, void* stream);
int bb_guided_loss_fused(const bb_guided_loss_args* a, void* stream);

/* The CNN's 3x3 / padding-1 convolutions over 8x8 boards (network.py:75-117,
 * ResidualBlock network.py:14-30; nn.Conv2d.forward and its autograd
 * backward) under bf16 autocast, for the layers with 64 or 128 channels in and
 * out.  Activations are bf16 NHWC (channels_last) [N][8][8][C], 16-byte
 * aligned; accumulation is f32.  bb_conv3x3_prep casts the nn.Conv2d weight
 * f32 [cout][cin][3][3] (w_layout 0) or [cout][3][3][cin] (w_layout 1, a
 * channels_last parameter) to bf16 (round to nearest even, as autocast) in two
 * images: d_wf [9][cout][cin] for the forward and d_wd [9][cin][cout], taps
 * reversed, for the data gradient.  bb_conv3x3_forward writes
 * y = conv(x, w) without bias (bf16 [N][8][8][cout]) from d_wf; the data
 * gradient is the same call on dy with d_wd and cin / cout swapped.
 * bb_conv3x3_wgrad writes the f32 weight gradient, in w_layout, of
 * y = conv(x, w) for the output gradient dy; d_ws is caller scratch of
 * bb_conv3x3_workspace_bytes(N, cin, cout) bytes.  No atomics: results are
 * deterministic. */
int64_t bb_conv3x3_workspace_bytes(int32_t N, int32_t cin, int32_t cout);
int bb_conv3x3_prep(const float* d_w, int32_t cin, int32_t cout, int32_t w_layout, void* d_wf, void* d_wd,
                    void* stream);
/* bb_conv3x3_prep for num_layers <= 16 layers in one launch (host arrays of
 * per-layer device pointers and sizes). */
int bb_conv3x3_prep_multi(int32_t num_layers, const float* const* h_w, const int32_t* h_cin,
                          const int32_t* h_cout, const int32_t* h_w_layout, void* const* h_wf,
                          void* const* h_wd, void* stream);
int bb_conv3x3_forward(const void* d_x, const void* d_w, int32_t N, int32_t cin, int32_t cout, void* d_y,
                       void* stream);
/* bb_conv3x3_forward plus a bf16 NHWC tensor d_add of y's shape, added to the
 * bf16-rounded convolution and rounded again (torch's bf16 add): the data
 * gradient of a ResidualBlock's first convolution with the identity path's
 * gradient folded in (network.py:14-30). */
int bb_conv3x3_forward_add(const void* d_x, const void* d_w, int32_t N, int32_t cin, int32_t cout,
                           const void* d_add, void* d_y, void* stream);
/* bb_conv3x3_forward that also writes, from its store pass, the following BatchNorm's batch-statistics
 * partials: per workgroup and output channel the f64 sum and sum of squares of the stored bf16 outputs
 * (d_part [bb_conv3x3_stats_blocks(N, cout)][cout][3], the third 0), for bb_bn_fwd.part (ABI 8). */
int32_t bb_conv3x3_stats_blocks(int32_t N, int32_t cout);
int bb_conv3x3_forward_stats(const void* d_x, const void* d_w, int32_t N, int32_t cin, int32_t cout, void* d_y,
                             double* d_part, void* stream);
/* bb_conv3x3_forward run as a data gradient (y = dL/d(BatchNorm [+ ReLU] output)) that also writes that
 * BatchNorm's backward reduction partials: per workgroup and channel {sum g, sum g xhat, sum xhat}, g = y where
 * the forward's ReLU (relu != 0) passed, xhat = (bn_x - mean) invstd, bn_x the BatchNorm's bf16 NHWC input
 * (y's shape) and mean / invstd / weight / bias its forward's (bb_bn_bwd.part; ABI 8). */
int bb_conv3x3_forward_bstats(const void* d_x, const void* d_w, int32_t N, int32_t cin, int32_t cout, void* d_y,
                              const void* d_bn_x, const float* d_mean, const float* d_invstd, const float* d_weight,
                              const float* d_bias, int32_t relu, double* d_part, void* stream);
int bb_conv3x3_wgrad(const void* d_x, const void* d_dy, int32_t N, int32_t cin, int32_t cout, float* d_ws,
                     int32_t w_layout, float* d_dw, void* stream);
/* bb_conv3x3_wgrad in two parts (ABI 8): the partial-sum kernel into d_ws, then the fixed-order sum of its
 * bb_conv3x3_wgrad_chunks(N, cin, cout) chunks into d_dw (alone, or as bb_bn_bwd.reduce); together
 * bit-identical to bb_conv3x3_wgrad. */
int32_t bb_conv3x3_wgrad_chunks(int32_t N, int32_t cin, int32_t cout);
int bb_conv3x3_wgrad_partial(const void* d_x, const void* d_dy, int32_t N, int32_t cin, int32_t cout, float* d_ws,
                             void* stream);
int bb_conv3x3_wgrad_reduce(const float* d_ws, int32_t chunks, int32_t cin, int32_t cout, int32_t w_layout,
                            float* d_dw, void* stream);

/* The same 3x3 convolutions in fp32 (no autocast: the reference's own precision), for (cin, cout) =
 * (128, 128), (64, 128) and (128, 64) (the last is the data gradient of the 64 -> 128 layer).  Every output
 * is the fp64 sum of 16-product fp32 MFMA chains, rounded to fp32 once (csrc/bb_conv32.hip): within
 * north_star's 1e-5 after the batch-statistics BatchNorms where MIOpen's 1,152-product order was not
 * (network.py:75-182 in train mode, scripts/train.py:122).  Activations f32 NHWC [N][8][8][C], 16-byte
 * aligned.  bb_conv3x3_f32_prep writes the f32 weight images d_wf [9][cout][cin] (forward) and
 * d_wd [9][cin][cout] (taps reversed, data gradient) from w_layout 0 / 1 as bb_conv3x3_prep; either output
 * may be NULL.  bb_conv3x3_f32_forward writes y = conv(x, w) without bias from d_wf; the data gradient is
 * the same call on dy with d_wd and cin / cout swapped.  Deterministic. */
int bb_conv3x3_f32_prep(const float* d_w, int32_t cin, int32_t cout, int32_t w_layout, float* d_wf, float* d_wd,
                        void* stream);
int bb_conv3x3_f32_forward(const float* d_x, const float* d_w, int32_t N, int32_t cin, int32_t cout, float* d_y,
                           void* stream);
/* nn.Linear's forward y = x w^T + bias in fp32 with the same accumulation (fp64 sum of 16-product fp32 MFMA
 * chains, the bias added in fp64, one rounding): the K = 8,192 first fc_encoder layer of the rollout's
 * forward (network.py:89-117, 135-182).  x [M][K], w [N][K] (nn.Linear.weight), y [M][N], all row-major and
 * 16-byte aligned; bias [N] or NULL; N % 128 == 0, K % 32 == 0.  Deterministic. */
int bb_linear_f32(const float* d_x, const float* d_w, const float* d_bias, int32_t M, int32_t N, int32_t K,
                  float* d_y, void* stream);

/* The end of the PPO minibatch step (PPOAgent.update, ppo.py:400-401):
 * nn.utils.clip_grad_norm_(params, max_norm) followed by
 * torch.optim.Adam(lr, betas, eps).step() (weight decay 0, no amsgrad), over
 * up to BB_OPT_MAX_TENSORS f32 parameter tensors given as host arrays of device
 * pointers: parameter, gradient, exp_avg, exp_avg_sq (same layout and numel
 * each) and Adam's per-tensor step count (f32 scalar on the device, incremented
 * first, as torch's fused / capturable Adam keeps it).  The gradient is scaled
 * by min(max_norm / (||g||_2 + 1e-6), 1) in place, as clip_grad_norm_ leaves
 * it; ||g|| over all tensors is written to d_total_norm when non-NULL.  d_ws is
 * caller scratch of bb_adam_clip_workspace_bytes(num_tensors, h_numel) bytes
 * (16-byte aligned).  Three kernel launches on `stream`; the tensor table is
 * passed by value, so the launches can be captured into a HIP graph.  The norm
 * is summed in a fixed order: deterministic.
 * Guard: zero d_ws once before the first call.  Then uint32 word
 * BB_ADAM_GUARD_WORD of d_ws holds 1 + the first chunk (BB_ADAM_CHUNK gradient
 * elements, chunks numbered across the tensors in table order) whose sum of
 * squares was non-finite or above 1e16.  The next word counts such chunks.
 * Both are sticky until the caller clears them.  The update itself is not
 * altered (runtime/kernels.py adam_guard_check reads and clears them). */
#define BB_OPT_MAX_TENSORS 48
#define BB_ADAM_GUARD_WORD 2
#define BB_ADAM_CHUNK 2048
int64_t bb_adam_clip_workspace_bytes(int32_t num_tensors, const int64_t* h_numel);
int bb_adam_clip_step(int32_t num_tensors, float* const* h_param, float* const* h_grad,
                      float* const* h_exp_avg, float* const* h_exp_avg_sq, float* const* h_step,
                      const int64_t* h_numel, double lr, double beta1, double beta2, double eps,
                      float max_norm, double* d_ws, float* d_total_norm, void* stream);

/* bf16 autocast's parameter casts for the CNN's nn.Linear layers
 * (network.py:89-117 under torch.autocast), all tensors in one launch: dir 0
 * casts f32 -> bf16 (round to nearest even), dir 1 bf16 -> f32 (their
 * gradients).  h_perm_c (NULL = none) > 0 marks a tensor of O rows whose f32
 * side is [O][perm_c][perm_hw] and whose bf16 side is [O][perm_hw][perm_c] (the
 * first FC weight against a channels_last flatten); perm_c * perm_hw <= 8192. */
int bb_cast_multi(int32_t num_tensors, int32_t dir, const void* const* h_src, void* const* h_dst,
                  const int64_t* h_numel, const int32_t* h_perm_c, const int32_t* h_perm_hw, void* stream);

/* The CNN's bf16 Linear tails (network.py:89-117: nn.Linear -> nn.ReLU -> nn.Dropout under autocast), not
 * part of the env boundary.
 * bb_dropout_forward: nn.Dropout(p)'s training forward, in place over n bf16 values (n % 8 == 0, 16-byte
 * aligned): y * (1 / (1 - p)) where the element is kept, else 0.  Element i is dropped when draw i % 4 of
 * Philox4x32-10(counter = (i / 4, offset), key = seed) is below p * 2^32.  d_rng is a device int64[4]
 * {seed, offset, 0, 0}: the launch reads (seed, offset), and the last of its workgroups advances offset by
 * one (words 2-3 are its scratch and stay 0 between launches), so every launch -- and every replay of a
 * captured graph -- draws a new mask.  One launch.
 * bb_linear_bgrad: the backward of y = dropout(relu(x w^T + b)) up to its GEMMs.  d_yd = the saved output
 * (bf16 [rows][cols]): g = dy * scale where yd > 0, else 0 (scale = the dropout's 1 / (1 - p), or 1), written
 * to d_g; d_yd = NULL: g = dy (plain Linear, nothing written).  d_db[c] = sum over rows of g[., c], f32 sums
 * in a fixed order rounded to bf16 (deterministic).  One launch: row chunks of 64 columns each publish
 * partial sums to d_ws (bb_linear_bgrad_workspace_bytes(rows, cols) bytes) and the last chunk to finish adds
 * them; d_cnt holds bb_linear_bgrad_counters(cols) uint32 counters that must be zero before the first launch
 * and are zero again after each (the launch re-arms them) -- one counter block per stream: launches that run
 * concurrently must not share one. */
int bb_dropout_forward(void* d_y, int64_t n, float p, int64_t* d_rng, void* stream);

/* The CNN's input layer, conv 4 -> 64 3x3 pad 1 over 8x8 boards (network.py:75-87, the first nn.Conv2d, without
 * its bias: the BatchNorm after it adds that) under bf16 autocast, not part of the env boundary.  x: N boards
 * of f32 [4][8][8] (x_nhwc 0) or [8][8][4] (x_nhwc 1, channels_last), 16-byte aligned; w: f32 [64][4][3][3]
 * (wl 0) or [64][3][3][4] (wl 1).  x and w are rounded to bf16 as autocast casts them, products summed in f32.
 * bb_conv_in_forward: y = bf16 [N][8][8][64] (NHWC).  One launch.
 * bb_conv_in_wgrad: dw (f32, w's layout) = sum over boards and pixels of dy (bf16 NHWC [N][8][8][64]) times
 * the bf16 input, f32 sums: per-workgroup partials in d_ws (bb_conv_in_wgrad_workspace_bytes(N) bytes) added
 * in a fixed order (deterministic).  Two launches. */
int64_t bb_conv_in_wgrad_workspace_bytes(int32_t N);
int bb_conv_in_forward(const float* d_x, int32_t x_nhwc, const float* d_w, int32_t wl, int32_t N, void* d_y,
                       void* stream);
int bb_conv_in_wgrad(const float* d_x, int32_t x_nhwc, const void* d_dy, int32_t N, float* d_ws, int32_t wl,
                     float* d_dw, void* stream);
/* bb_conv_in_forward plus bb_conv3x3_prep_multi's weight images of the other layers (same table arguments) in one
 * launch: both run at the start of the CNN's forward and are independent. */
int bb_conv_in_forward_prep(const float* d_x, int32_t x_nhwc, const float* d_w, int32_t wl, int32_t N, void* d_y,
                            int32_t count, const float* const* h_w, const int32_t* h_cin, const int32_t* h_cout,
                            const int32_t* h_w_layout, void* const* h_wf, void* const* h_wd, void* stream);
/* bb_linear_wgrad: a Linear's weight gradient dW = g^T x (g bf16 [rows][N], x bf16 [rows][K] with row stride
 * ldx >= K a multiple of 8, dW bf16 [N][K], all row-major; N and K multiples of 32, 16-byte aligned rows, rows <= 16384), f32 sums in a fixed order
 * rounded once (deterministic).  One launch: splits of 256 rows publish 32 x 32 partials to d_ws
 * (bb_linear_wgrad_workspace_bytes(rows, N, K) bytes) and the last split of a tile adds them; d_cnt: the
 * bb_linear_wgrad_counters(N, K) uint32 counters, zero before and after each launch (as bb_linear_bgrad's,
 * and the same counter block may serve both on one stream). */
/* bb_linear_n1_forward / _backward: a bf16 Linear with one output (the value head's Linear(128, 1)), x bf16
 * [rows][K] with row stride ldx (>= K, a multiple of 8), w bf16 [K], b bf16 [1] (NULL: none), K a multiple of
 * 8, 16-byte aligned.  Forward: y[r] = bf16(sum_k x[r][k] w[k] + b), f32 sums.  Backward: dx[r][k] = bf16(gy[r] w[k]), dW[k] = sum_r gy[r] x[r][k],
 * db = sum_r gy[r] (d_db NULL: skipped), f32 sums in a fixed order rounded to bf16; row chunks publish
 * partials to d_ws (bb_linear_n1_workspace_bytes(rows, K) bytes) with bb_linear_n1_counters(K) zeroed
 * counters in d_cnt (as bb_linear_bgrad).  One launch each.  Both size queries return -1 for a K that is not a
 * positive multiple of 8. */
int64_t bb_linear_n1_workspace_bytes(int32_t rows, int32_t K);
int32_t bb_linear_n1_counters(int32_t K);
int bb_linear_n1_forward(const void* d_x, const void* d_w, const void* d_b, int32_t rows, int32_t K, int32_t ldx,
                         void* d_y, void* stream);
int bb_linear_n1_backward(const void* d_gy, const void* d_x, const void* d_w, int32_t rows, int32_t K, int32_t ldx,
                          void* d_dx, void* d_dw, void* d_db, float* d_ws, uint32_t* d_cnt, void* stream);
int64_t bb_linear_wgrad_workspace_bytes(int32_t rows, int32_t N, int32_t K);
int32_t bb_linear_wgrad_counters(int32_t N, int32_t K);
int bb_linear_wgrad(const void* d_g, const void* d_x, int32_t rows, int32_t N, int32_t K, int32_t ldx, void* d_dw,
                    float* d_ws, uint32_t* d_cnt, void* stream);
int64_t bb_linear_bgrad_workspace_bytes(int32_t rows, int32_t cols);
int32_t bb_linear_bgrad_counters(int32_t cols);
int bb_linear_bgrad(const void* d_dy, const void* d_yd, int32_t rows, int32_t cols, float scale, void* d_g,
                    void* d_db, float* d_ws, uint32_t* d_cnt, void* stream);
/* bb_linear_bgrad over two layers' output gradients side by side (ABI 8): columns [0, split) of dy come from d_dy
 * ([rows][split]), columns [split, cols) from d_dy2 ([rows][cols - split]); d_yd, d_g are [rows][cols] (the
 * policy and value heads' first layers as one GEMM). */
int bb_linear_bgrad2(const void* d_dy, const void* d_dy2, int32_t split, const void* d_yd, int32_t rows, int32_t cols,
                     float scale, void* d_g, void* d_db, float* d_ws, uint32_t* d_cnt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BBVEC_H */
