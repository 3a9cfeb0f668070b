// bb_look_rules.h -- the argument rules of the thirty-one lookahead entry points of include/bbvec.h, one copy for
// both backends (csrc/bb_capi.cpp and csrc/bb_host.cpp).  Plain C++, nothing from HIP.
//
// Each function returns the rule an argument set breaks, as the text that follows "<entry point>: " in
// bb_last_error, or nullptr when the call is accepted.  A refusal is BB_ERR_ARG and comes before any HIP call.
// The handle forms check the handle themselves, first: a NULL env is a bare BB_ERR_ARG with no text.
//
// Asymmetries that are part of the ABI as it stands: bb_afterstates_pos, bb_greedy_actions(_each)_pos and
// bb_plan_actions(_each)_pos refuse n == 0 and answer every broken rule with one text; bb_plan_values_pos accepts n == 0
// (and does nothing) and names the rule that broke, and so do bb_safe_mask_pos, bb_refill_census_pos,
// bb_refill_values_pos, bb_play_plan_pos, bb_board_terms_pos, bb_plan_actions_ext_pos, bb_plan_values_ext_pos,
// bb_refill_values_ext_pos, bb_plan2_values_pos and bb_playout_values_pos.
#pragma once
#include <stdint.h>

#include "../../include/bbvec.h"

namespace bb_look_rules {

inline bool no_positions(const bb_positions* pos) { return !pos || !pos->board || !pos->hand; }
inline bool bad_depth(int32_t depth) { return depth < 1 || depth > 3; }

inline const char* afterstates(const bb_afterstate_out* out) { return out ? nullptr : "out is NULL"; }
inline const char* afterstates_pos(const bb_positions* pos, int32_t n, const bb_reward_cfg* cfg,
                                   const bb_afterstate_out* out) {
  return no_positions(pos) || n <= 0 || !cfg || !out ? "positions (board, hand), n > 0, cfg and out are required"
                                                     : nullptr;
}

inline const char* greedy_actions(const bb_greedy_weights* w, const int32_t* d_action) {
  return !w || !d_action ? "weights and d_action are required" : nullptr;
}
inline const char* greedy_actions_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w,
                                      const int32_t* d_action) {
  return no_positions(pos) || n <= 0 || !w || !d_action
             ? "positions (board, hand), n > 0, weights and d_action are required"
             : nullptr;
}

inline const char* plan_actions(const bb_greedy_weights* w, int32_t depth, const bb_plan_out* out) {
  return !w || !out || !out->action || bad_depth(depth) ? "weights, depth in 1..3 and out->action are required"
                                                        : nullptr;
}
inline const char* plan_actions_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t depth,
                                    const bb_plan_out* out) {
  return no_positions(pos) || n <= 0 || !w || !out || !out->action || bad_depth(depth)
             ? "positions (board, hand), n > 0, weights, depth in 1..3 and out->action are required"
             : nullptr;
}

// the per-position forms (bb_*_each): the uniform form's rule with "weight rows" for "weights"
inline const char* greedy_actions_each(const bb_greedy_weights* d_w, const int32_t* d_action) {
  return !d_w || !d_action ? "weight rows and d_action are required" : nullptr;
}
inline const char* greedy_actions_each_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* d_w,
                                           const int32_t* d_action) {
  return no_positions(pos) || n <= 0 || !d_w || !d_action
             ? "positions (board, hand), n > 0, weight rows and d_action are required"
             : nullptr;
}
inline const char* plan_actions_each(const bb_greedy_weights* d_w, int32_t depth, const bb_plan_out* out) {
  return !d_w || !out || !out->action || bad_depth(depth) ? "weight rows, depth in 1..3 and out->action are required"
                                                          : nullptr;
}
inline const char* plan_actions_each_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* d_w,
                                         int32_t depth, const bb_plan_out* out) {
  return no_positions(pos) || n <= 0 || !d_w || !out || !out->action || bad_depth(depth)
             ? "positions (board, hand), n > 0, weight rows, depth in 1..3 and out->action are required"
             : nullptr;
}

inline const char* plan_values(const bb_greedy_weights* w, int32_t depth, const bb_plan_values_out* out) {
  if (!w) return "weights are NULL";
  if (!out) return "out is NULL";
  if (!out->q && !out->rest && !out->leaves && !out->safe) return "all four outputs are NULL";
  if (bad_depth(depth)) return "depth must be 1..3";
  return nullptr;
}
inline const char* plan_values_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t depth,
                                   const bb_plan_values_out* out) {
  if (no_positions(pos)) return "positions (board, hand) are NULL";
  if (n < 0) return "n is negative";
  return plan_values(w, depth, out);
}

inline const char* safe_mask(int32_t mode, const uint64_t* d_mask) {
  if (!d_mask) return "d_mask is NULL";
  if (mode < BB_SAFE_WORDS || mode > BB_SAFE_OR_LEGAL) return "mode must be 0..1";
  return nullptr;
}
inline const char* safe_mask_pos(const bb_positions* pos, int32_t n, int32_t mode, const uint64_t* d_mask) {
  if (no_positions(pos)) return "positions (board, hand) are NULL";
  if (n < 0) return "n is negative";
  return safe_mask(mode, d_mask);
}

// the refill census reads a board column alone (no bb_positions) and, like bb_plan_values_pos, accepts n == 0
inline const char* refill_census(const bb_census_out* out) {
  if (!out) return "out is NULL";
  if (!out->count && !out->solvable) return "both outputs are NULL";
  return nullptr;
}
inline const char* refill_census_pos(const uint64_t* board, int32_t n, const bb_census_out* out) {
  if (!board) return "board is NULL";
  if (n < 0) return "n is negative";
  return refill_census(out);
}

// the dealt next-hand values: board (and combo, stream) columns, no bb_positions; n == 0 is accepted
inline const char* refill_values(const bb_greedy_weights* w, int32_t depth, int32_t deals,
                                 const bb_refill_values_out* out) {
  if (!w) return "weights are NULL";
  if (!out) return "out is NULL";
  if (!out->hand && !out->value && !out->attempts) return "all three outputs are NULL";
  if (bad_depth(depth)) return "depth must be 1..3";
  if (deals < 1 || deals > BB_REFILL_MAX_DEALS) return "deals must be 1..1024";
  return nullptr;
}
inline const char* refill_values_pos(const uint64_t* board, int32_t n, const bb_greedy_weights* w, int32_t depth,
                                     int32_t deals, const bb_refill_values_out* out) {
  if (!board) return "board is NULL";
  if (n < 0) return "n is negative";
  return refill_values(w, depth, deals, out);
}

inline const char* play_plan_pos(const bb_positions* pos, int32_t n, const int32_t* plan, const bb_play_plan_out* out) {
  if (no_positions(pos)) return "positions (board, hand) are NULL";
  if (n < 0) return "n is negative";
  if (!plan) return "d_plan is NULL";
  if (!out) return "out is NULL";
  if (!out->board && !out->hand && !out->combo && !out->lines && !out->score && !out->status)
    return "all six outputs are NULL";
  return nullptr;
}

// the shape terms of a board column: as the refill census, n == 0 is accepted
inline const char* board_terms(const int32_t* d_terms) { return d_terms ? nullptr : "d_terms is NULL"; }
inline const char* board_terms_pos(const uint64_t* board, int32_t n, const int32_t* d_terms) {
  if (!board) return "board is NULL";
  if (n < 0) return "n is negative";
  return board_terms(d_terms);
}

// the search with the shape terms: rows of bb_eval_weights, shared (w_stride 0) or one per position (1)
inline const char* plan_actions_ext(const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                                    const bb_plan_out* out) {
  if (!d_w) return "weight rows are NULL";
  if (w_stride != 0 && w_stride != 1) return "w_stride must be 0 or 1";
  if (bad_depth(depth)) return "depth must be 1..3";
  if (!out) return "out is NULL";
  if (!out->action) return "out->action is NULL";
  return nullptr;
}
inline const char* plan_actions_ext_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w,
                                        int64_t w_stride, int32_t depth, const bb_plan_out* out) {
  if (no_positions(pos)) return "positions (board, hand) are NULL";
  if (n < 0) return "n is negative";
  return plan_actions_ext(d_w, w_stride, depth, out);
}

// the per-action values and the dealt next-hand values with the shape terms: the rules of bb_plan_values /
// bb_refill_values with "weight rows" for "weights", and the stride rule of bb_plan_actions_ext
inline const char* plan_values_ext(const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                                   const bb_plan_values_out* out) {
  if (!d_w) return "weight rows are NULL";
  if (w_stride != 0 && w_stride != 1) return "w_stride must be 0 or 1";
  if (!out) return "out is NULL";
  if (!out->q && !out->rest && !out->leaves && !out->safe) return "all four outputs are NULL";
  if (bad_depth(depth)) return "depth must be 1..3";
  return nullptr;
}
inline const char* plan_values_ext_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w,
                                       int64_t w_stride, int32_t depth, const bb_plan_values_out* out) {
  if (no_positions(pos)) return "positions (board, hand) are NULL";
  if (n < 0) return "n is negative";
  return plan_values_ext(d_w, w_stride, depth, out);
}
inline const char* refill_values_ext(const bb_eval_weights* d_w, int64_t w_stride, int32_t depth, int32_t deals,
                                     const bb_refill_values_out* out) {
  if (!d_w) return "weight rows are NULL";
  if (w_stride != 0 && w_stride != 1) return "w_stride must be 0 or 1";
  if (!out) return "out is NULL";
  if (!out->hand && !out->value && !out->attempts) return "all three outputs are NULL";
  if (bad_depth(depth)) return "depth must be 1..3";
  if (deals < 1 || deals > BB_REFILL_MAX_DEALS) return "deals must be 1..1024";
  return nullptr;
}
inline const char* refill_values_ext_pos(const uint64_t* board, int32_t n, const bb_eval_weights* d_w,
                                         int64_t w_stride, int32_t depth, int32_t deals,
                                         const bb_refill_values_out* out) {
  if (!board) return "board is NULL";
  if (n < 0) return "n is negative";
  return refill_values_ext(d_w, w_stride, depth, deals, out);
}

// the two-hand decision (bb_plan2_values): the workspace of n positions, K candidates and `deals` deals as byte
// offsets, the 8-byte arrays first.  Both backends carve the caller's scratch with it, and bb_plan2_work_bytes is
// its `bytes`.
struct Plan2Layout {
  int64_t q, board, moved, value, rest, combo, cand, status, bytes;
  Plan2Layout(int64_t n, int64_t k, int64_t deals) {
    int64_t at = 0;
    q = at, at += n * 192 * 8;            // int64  [n][192]
    board = at, at += n * k * 8;          // uint64 [n][K]
    moved = at, at += n * k * 8;          // int64  [n][K]
    value = at, at += n * k * deals * 8;  // int64  [n][K][deals]
    rest = at, at += n * 192 * 4;         // int32  [n][192]
    combo = at, at += n * k * 4;          // int32  [n][K]
    cand = at, at += n * k * 4;           // int32  [n][K]
    status = at, at += n * k * 4;         // int32  [n][K]
    bytes = (at + 7) & ~(int64_t)7;
  }
};
inline bool bad_plan2_sizes(int32_t n, int32_t candidates, int32_t deals) {
  return n < 0 || candidates < 1 || candidates > 192 || deals < 1 || deals > BB_REFILL_MAX_DEALS;
}
inline int64_t plan2_work_bytes(int32_t n, int32_t candidates, int32_t deals) {
  return bad_plan2_sizes(n, candidates, deals) ? -1 : Plan2Layout(n, candidates, deals).bytes;
}
// n: the positions of the _pos form, the handle's envs of the handle form
inline const char* plan2_values(int32_t n, const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                                int32_t candidates, int32_t deals, const void* d_work, int64_t work_bytes,
                                const bb_plan2_out* out) {
  if (n < 0) return "n is negative";
  if (!d_w) return "weight rows are NULL";
  if (w_stride != 0 && w_stride != 1) return "w_stride must be 0 or 1";
  if (!out) return "out is NULL";
  if (!out->action && !out->q2 && !out->cand && !out->status && !out->value) return "all five outputs are NULL";
  if (bad_depth(depth)) return "depth must be 1..3";
  if (candidates < 1 || candidates > 192) return "candidates must be 1..192";
  if (deals < 1 || deals > BB_REFILL_MAX_DEALS) return "deals must be 1..1024";
  if (!d_work) return "d_work is NULL";
  if (work_bytes < plan2_work_bytes(n, candidates, deals)) return "work_bytes is below bb_plan2_work_bytes";
  return nullptr;
}
inline const char* plan2_values_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w, int64_t w_stride,
                                    int32_t depth, int32_t candidates, int32_t deals, const void* d_work,
                                    int64_t work_bytes, const bb_plan2_out* out) {
  if (no_positions(pos)) return "positions (board, hand) are NULL";
  return plan2_values(n, d_w, w_stride, depth, candidates, deals, d_work, work_bytes, out);
}

// the dealt playouts (bb_playout_values): the rules of bb_refill_values_ext with playouts for deals, and the hand count
inline const char* playout_values(const bb_eval_weights* d_w, int64_t w_stride, int32_t depth, int32_t playouts,
                                  int32_t hands, const bb_playout_out* out) {
  if (!d_w) return "weight rows are NULL";
  if (w_stride != 0 && w_stride != 1) return "w_stride must be 0 or 1";
  if (!out) return "out is NULL";
  if (!out->value && !out->score && !out->lines && !out->plies && !out->hands && !out->status && !out->board &&
      !out->combo && !out->hand)
    return "all nine outputs are NULL";
  if (bad_depth(depth)) return "depth must be 1..3";
  if (playouts < 1 || playouts > BB_REFILL_MAX_DEALS) return "playouts must be 1..1024";
  if (hands < 1 || hands > BB_PLAYOUT_MAX_HANDS) return "hands must be 1..256";
  return nullptr;
}
inline const char* playout_values_pos(const uint64_t* board, int32_t n, const bb_eval_weights* d_w, int64_t w_stride,
                                      int32_t depth, int32_t playouts, int32_t hands, const bb_playout_out* out) {
  if (!board) return "board is NULL";
  if (n < 0) return "n is negative";
  return playout_values(d_w, w_stride, depth, playouts, hands, out);
}

}  // namespace bb_look_rules
