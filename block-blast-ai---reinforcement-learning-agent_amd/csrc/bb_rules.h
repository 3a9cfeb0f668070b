// bb_rules.h -- the rules of a Block Blast move that the HIP kernels and the host backend share.
//
// One definition each of: the board constants, the packed hand word, count_holes, the score of a move, the
// fp64 shaped reward, what a placement leads to (After) with its greedy value terms and aux word, and the
// bb_info record.  Plain C++ with no HIP include: g++ compiles it for libbbvec_host.so, hipcc for host and
// device of libbbvec.so.  Every function names the reference code whose semantics it reproduces.
//
// Deliberately not here: clear_full, anchors_of / dilate and the piece tables.  The device versions are tuned
// (byte-permute, Minkowski program) and the host's plain loops are their independent check in the
// cross-backend tests; likewise the PCG64 / Philox streams, the hand solver and the search structure.
#pragma once
#include <stdint.h>

#include "../../include/bbvec.h"

#if defined(__HIPCC__)
#define BB_RULE __host__ __device__ inline
#else
#define BB_RULE inline
#endif

namespace bb {

constexpr int kPieces = 37;
constexpr int kHand = 3;

constexpr uint64_t kRow0 = 0x00000000000000FFull;
constexpr uint64_t kRow7 = 0xFF00000000000000ull;
constexpr uint64_t kCol0 = 0x0101010101010101ull;
constexpr uint64_t kCol7 = 0x8080808080808080ull;
constexpr uint64_t kCenter = 0x00003C3C3C3C0000ull;  // rows 2-5 x cols 2-5 (board.py:242)

// --------------------------------------------------------------------------
// Packed hand word (also the host-visible layout, see bbvec.h bb_state_view):
// 3 x 6-bit piece ids | used << 18 | over << 21 | has_uint32 << 22.
// --------------------------------------------------------------------------
constexpr uint32_t kHandIds = 0x3FFFFu;
constexpr int kHandUsedShift = 18, kHandOverShift = 21, kHandHas32Shift = 22;

BB_RULE uint32_t hand_id(uint32_t h, int slot) { return (h >> (6 * slot)) & 63u; }
BB_RULE uint32_t hand_ids(uint32_t h) { return h & kHandIds; }
BB_RULE uint32_t hand_used(uint32_t h) { return (h >> kHandUsedShift) & 7u; }
BB_RULE bool hand_over(uint32_t h) { return (h >> kHandOverShift) & 1u; }
BB_RULE bool hand_has32(uint32_t h) { return (h >> kHandHas32Shift) & 1u; }
BB_RULE uint32_t hand_pack(uint32_t a, uint32_t b, uint32_t c, uint32_t used, bool over, bool has32) {
  return a | (b << 6) | (c << 12) | (used << kHandUsedShift) | ((uint32_t)over << kHandOverShift) |
         ((uint32_t)has32 << kHandHas32Shift);
}
// a freshly drawn hand from its id word (has32: 0 or 1): nothing used, not over
BB_RULE uint32_t hand_new(uint32_t ids, uint32_t has32) { return ids | (has32 << kHandHas32Shift); }
// slot p marked used
BB_RULE uint32_t hand_use(uint32_t h, int p) { return h | (1u << (kHandUsedShift + p)); }
// the hand a move leaves behind: ids and has_uint32 kept, the used bits replaced, not over
BB_RULE uint32_t hand_with_used(uint32_t h, uint32_t used) {
  return (h & kHandIds) | (used << kHandUsedShift) | (h & (1u << kHandHas32Shift));
}
BB_RULE uint32_t hand_clear_used(uint32_t h) { return h & ~(7u << kHandUsedShift); }
BB_RULE uint32_t hand_set_over(uint32_t h) { return h | (1u << kHandOverShift); }

// Board.count_holes (board.py:195-216): empty cells whose four neighbours are
// all filled or off-board.
BB_RULE int count_holes(uint64_t B) {
  const uint64_t n = (B << 8) | kRow0;
  const uint64_t s = (B >> 8) | kRow7;
  const uint64_t w = ((B << 1) & ~kCol0) | kCol0;
  const uint64_t e = ((B >> 1) & ~kCol7) | kCol7;
  return __builtin_popcountll(~B & n & s & w & e);
}

// --------------------------------------------------------------------------
// Shape terms of a board (bbvec.h bb_board_terms / bb_eval_weights): what the board can still take.
// --------------------------------------------------------------------------
// perimeter: the pairs (empty cell, side) whose neighbour across that side is filled or off the board -- the four
// neighbour boards of count_holes, counted side by side instead of and-ed.
BB_RULE int perimeter(uint64_t B) {
  const uint64_t n = (B << 8) | kRow0;
  const uint64_t s = (B >> 8) | kRow7;
  const uint64_t w = ((B << 1) & ~kCol0) | kCol0;
  const uint64_t e = ((B >> 1) & ~kCol7) | kCol7;
  return __builtin_popcountll(~B & n) + __builtin_popcountll(~B & s) + __builtin_popcountll(~B & w) +
         __builtin_popcountll(~B & e);
}

// Where pieces fit (Board.can_place, board.py:71-93), as anchor boards.  With E the empty cells, `a` `b` `c` are E
// seen 0, 1, 2 columns to the right of the anchor -- bit (r, c) of b says (r, c+1) is on the board and empty -- and
// X >> 8k is X seen k rows below (rows off the board shift in as zeros: not empty).  A piece's anchor board is the
// and of one such board per cell; the runs h2..h5 (cells to the right) and v2..v5 (cells below) are shared.
struct Fit {
  uint64_t a, b, c, h2, h3, h4, h5, v2, v3, v4, v5;
};
BB_RULE Fit fit_runs(uint64_t B) {
  Fit f;
  const uint64_t E = ~B;
  f.a = E;
  f.b = (E >> 1) & ~kCol7;
  f.c = (E >> 2) & ~(kCol7 | (kCol7 >> 1));
  f.h2 = f.a & f.b;
  f.h3 = f.h2 & f.c;
  f.h4 = f.h3 & ((E >> 3) & (kCol0 * 0x1Full));
  f.h5 = f.h4 & ((E >> 4) & (kCol0 * 0x0Full));
  f.v2 = E & (E >> 8);
  f.v3 = f.v2 & (E >> 16);
  f.v4 = f.v3 & (E >> 24);
  f.v5 = f.v4 & (E >> 32);
  return f;
}
// the anchors of SQUARE_3x3 (piece 36)
BB_RULE uint64_t square3_anchors(const Fit& f) { return f.h3 & (f.h3 >> 8) & (f.h3 >> 16); }

BB_RULE int room3(uint64_t B) { return __builtin_popcountll(square3_anchors(fit_runs(B))); }
BB_RULE int room5(uint64_t B) {
  const Fit f = fit_runs(B);
  return __builtin_popcountll(f.h5) + __builtin_popcountll(f.v5);  // I5_H (15), I5_V (16)
}

// fits: the piece ids that fit somewhere.  A piece fits wherever a piece containing it fits, so where the 3x3 square
// fits, the 33 pieces inside a 3x3 box do and only the four long bars are left to test; otherwise each of the 33 is
// tested by its own anchor board (game/pieces.py names and cell sets, ids in the comments).
BB_RULE int fits_of(const Fit& f, uint64_t sq) {
  const int bars = (f.h4 != 0) + (f.v4 != 0) + (f.h5 != 0) + (f.v5 != 0);  // I_H 13, I_V 14, I5_H 15, I5_V 16
  if (sq != 0) return 33 + bars;
  const uint64_t a = f.a, b = f.b, c = f.c, h2 = f.h2, h3 = f.h3, v3 = f.v3;
  const uint64_t a1 = a >> 8, b1 = b >> 8, c1 = c >> 8, a2 = a >> 16, b2 = b >> 16, c2 = c >> 16;
  const uint64_t h21 = h2 >> 8, h31 = h3 >> 8;
  const uint64_t vb3 = b & b1 & b2;  // the column right of the anchor, three cells down
  const uint64_t bc = b & c;         // (0,1), (0,2)
  int k = bars;
  k += a != 0;                       //  0 SINGLE
  k += h2 != 0;                      //  1 DOMINO_H
  k += f.v2 != 0;                    //  2 DOMINO_V
  k += (a & b1) != 0;                //  3 DIAG2_TL_BR
  k += (b & a1) != 0;                //  4 DIAG2_TR_BL
  k += h3 != 0;                      //  5 TRIO_H
  k += v3 != 0;                      //  6 TRIO_V
  k += (a & b1 & c2) != 0;           //  7 DIAG3_TL_BR
  k += (c & b1 & a2) != 0;           //  8 DIAG3_TR_BL
  k += (a & h21) != 0;               //  9 TRIO_L1
  k += (h2 & b1) != 0;               // 10 TRIO_L2
  k += (h2 & a1) != 0;               // 11 TRIO_L3
  k += (b & h21) != 0;               // 12 TRIO_L4
  k += (h2 & h21) != 0;              // 17 O
  k += (b & h31) != 0;               // 18 T_UP
  k += (h3 & b1) != 0;               // 19 T_DOWN
  k += (v3 & b1) != 0;               // 20 T_LEFT
  k += (vb3 & a1) != 0;              // 21 T_RIGHT
  k += (bc & h21) != 0;              // 22 S_H
  k += (a & h21 & b2) != 0;          // 23 S_V
  k += (h2 & (bc >> 8)) != 0;        // 24 Z_H
  k += (b & h21 & a2) != 0;          // 25 Z_V
  k += (v3 & b2) != 0;               // 26 L_1
  k += (h3 & a1) != 0;               // 27 L_2
  k += (a & vb3) != 0;               // 28 L_3
  k += (c & h31) != 0;               // 29 L_4
  k += (vb3 & a2) != 0;              // 30 J_1
  k += (a & h31) != 0;               // 31 J_2
  k += (v3 & b) != 0;                // 32 J_3
  k += (h3 & c1) != 0;               // 33 J_4
  k += (h3 & h31) != 0;              // 34 RECT_2x3_H
  k += (h2 & h21 & (h2 >> 16)) != 0; // 35 RECT_2x3_V
  return k;                          // 36 SQUARE_3x3 does not fit here
}
BB_RULE int fits(uint64_t B) {
  const Fit f = fit_runs(B);
  return fits_of(f, square3_anchors(f));
}

// the four in the order of bb_board_terms
BB_RULE void board_terms(uint64_t B, int32_t out[4]) {
  const Fit f = fit_runs(B);
  const uint64_t sq = square3_anchors(f);
  out[0] = perimeter(B);
  out[1] = __builtin_popcountll(sq);
  out[2] = __builtin_popcountll(f.h5) + __builtin_popcountll(f.v5);
  out[3] = fits_of(f, sq);
}

// --------------------------------------------------------------------------
// Score of a move (engine.py:240-262, 406-429), select-only so that the branch-free move of the rollout kernel
// uses it as it is.  `lines` lines cleared at combo `combo`:
// --------------------------------------------------------------------------
BB_RULE int line_cap(int lines) { return lines < 4 ? lines : 4; }
// the combo multiplier: 1 without a clear
BB_RULE int combo_multiplier(int lines) { return lines > 0 ? line_cap(lines) : 1; }
// the combo after a move that clears, and after any move
BB_RULE int combo_next(int combo) { return combo + 1; }
BB_RULE int combo_after(int lines, int combo) { return lines > 0 ? combo_next(combo) : 0; }
// score_gained of a move that placed `ncells` cells; combo1 is the combo after the move (read only with a clear,
// so combo_next(combo) serves as well as combo_after(lines, combo))
BB_RULE int64_t score_gained(int ncells, int lines, int combo1) {
  const int cm = line_cap(lines);
  const int streak = combo1 + 1 < 8 ? combo1 + 1 : 8;  // post-increment combo (engine.py:261)
  // blocks_in_lines = lines * 8 (engine.py:427).  No select: without a clear the product is 0 by its factor
  // `lines`, and with at most 16 lines, cm <= 4 and streak <= 8 it fits 32 bits (a 64-bit product made the
  // compiler split the branch-free move into a diamond).
  return (int64_t)ncells + (int64_t)(lines * 8 * 10 * cm * streak);
}

// _calculate_reward of a legal move (block_blast_env.py:158-193) in fp64.  The operation order is the
// contract (it is the reference's, and the results are compared bit for bit); both libraries are built with
// -ffp-contract=off, so none of these pairs is fused.  center_tenth = cfg.center_bonus * 0.1; holes / centre
// are the post-move hole and filled-centre counts, prev the pre-move ones (_prev_holes | centre << 8).
// Select-only like score_gained, so that the rollout kernel's finalize stays one basic block: every term is
// computed, and a conditional step commits as R = cond ? R + term : R.  The sum is selected, never a zero
// addend, so a step that is taken performs exactly the reference's addition and one that is not leaves R's bits
// alone (R + 0.0 would turn -0.0 into +0.0).
//
// In two parts.  The head runs up to and including the combo bonus and depends only on the config, the piece's
// cell count (0..9) and the lines cleared (0..6, cm = combo_multiplier(lines)): kRewardHeads values per config,
// which the rollout kernel tabulates once per launch with this same function.  The tail adds the rest to it.
constexpr int kRewardLines = 7, kRewardHeads = 10 * kRewardLines;
BB_RULE int reward_head_index(int ncells, int lines) { return ncells * kRewardLines + lines; }

BB_RULE double reward_head(const bb_reward_cfg& cfg, int ncells, int lines, int cm) {
  double R = 0.0;
  R += (double)ncells * cfg.block_placed;
  R += cfg.survival_bonus;
  const bool cleared = lines > 0;
  double lr = (double)lines * cfg.line_clear_base;
  lr *= (double)cm;
  const double r_lines = R + lr;
  R = cleared ? r_lines : R;
  const double r_combo = R + (double)(cm - 1) * cfg.combo_multiplier_bonus;
  R = cleared && cm > 1 ? r_combo : R;
  return R;
}

BB_RULE double reward_tail(const bb_reward_cfg& cfg, double center_tenth, double R, bool over, int holes, int centre,
                           uint32_t prev) {
  const double r_over = R + cfg.game_over_penalty;
  R = over ? r_over : R;
  const int dh = holes - (int)(prev & 0xFFu);
  const double r_holes = R + (double)dh * cfg.hole_penalty;
  R = dh > 0 ? r_holes : R;
  const double r_centre = R + center_tenth;
  R = centre <= (int)(prev >> 8) ? r_centre : R;  // openness >= previous
  return R;
}

BB_RULE double move_reward(const bb_reward_cfg& cfg, double center_tenth, int ncells, int lines, int cm, bool over,
                           int holes, int centre, uint32_t prev) {
  return reward_tail(cfg, center_tenth, reward_head(cfg, ncells, lines, cm), over, holes, centre, prev);
}

// --------------------------------------------------------------------------
// One-ply lookahead (bbvec.h bb_afterstates / bb_greedy_actions / bb_plan_actions)
// --------------------------------------------------------------------------
// What one legal placement leads to (illegal: legal == false and the rest unspecified).
struct After {
  bool legal, dead, refill;
  uint64_t board;  // B' (after the clears)
  int ncells, lines, combo1, holes, centre, filled, mobility;
  int64_t gained;
};

// the reward of the placement, with game_over = dead
BB_RULE double after_reward(const After& a, const bb_reward_cfg& cfg, double center_tenth, uint32_t prev) {
  return move_reward(cfg, center_tenth, a.ncells, a.lines, combo_multiplier(a.lines), a.dead, a.holes, a.centre, prev);
}

// the aux word of bb_afterstate_out
BB_RULE uint32_t pack_aux(const After& a) {
  return 1u | ((uint32_t)a.dead << 1) | ((uint32_t)a.refill << 2) | ((uint32_t)a.lines << 8) |
         ((uint32_t)a.holes << 12) | ((uint32_t)a.centre << 19) | ((uint32_t)a.mobility << 24);
}

// The greedy value of a placement is move_terms + state_terms; a plan sums the move terms of its plies and
// adds the state terms of its last afterstate.
BB_RULE int64_t move_terms(const bb_greedy_weights& w, const After& a) {
  return (int64_t)w.lines * a.lines + (int64_t)w.score * a.gained;
}

BB_RULE int64_t state_terms(const bb_greedy_weights& w, const After& a) {
  return (int64_t)w.holes * a.holes + (int64_t)w.filled * a.filled + (int64_t)w.centre * a.centre +
         (int64_t)w.mobility * a.mobility + (int64_t)w.dead * (int)a.dead + (int64_t)w.refill * (int)a.refill;
}

// The same two under bb_eval_weights (bbvec.h bb_plan_actions_ext): the base terms, and on the state side the shape
// terms of the afterstate's board.  A term whose weight is 0 is not computed; the runs are formed once for the
// terms that need them.
static_assert(sizeof(bb_eval_weights) == 12 * sizeof(int32_t), "an extended weight row is twelve int32");
BB_RULE int64_t shape_terms(const bb_eval_weights& w, uint64_t B) {
  int64_t v = 0;
  if (w.perimeter != 0) v += (int64_t)w.perimeter * perimeter(B);
  if ((w.room3 | w.room5 | w.fits) != 0) {
    const Fit f = fit_runs(B);
    const uint64_t sq = square3_anchors(f);
    if (w.room3 != 0) v += (int64_t)w.room3 * __builtin_popcountll(sq);
    if (w.room5 != 0) v += (int64_t)w.room5 * (__builtin_popcountll(f.h5) + __builtin_popcountll(f.v5));
    if (w.fits != 0) v += (int64_t)w.fits * fits_of(f, sq);
  }
  return v;
}
BB_RULE int64_t move_terms(const bb_eval_weights& w, const After& a) { return move_terms(w.base, a); }
BB_RULE int64_t state_terms(const bb_eval_weights& w, const After& a) {
  return state_terms(w.base, a) + shape_terms(w, a.board);
}

// --------------------------------------------------------------------------
// The info record of one step (block_blast_env.py:266-288): totals after the move and before any auto-reset,
// then the move's own summary.
// --------------------------------------------------------------------------
BB_RULE bb_info make_info(int64_t score, int64_t gained, uint64_t board, int32_t moves, int32_t lines_tot,
                          int32_t max_combo, int32_t blocks, uint32_t hand, int holes, bool valid, bool term,
                          int nblk, int lines, int cm) {
  bb_info f;
  f.score = score;
  f.score_gained = gained;
  f.term_board = board;
  f.moves = moves;
  f.lines = lines_tot;
  f.max_combo = max_combo;
  f.blocks = blocks;
  f.term_hand = hand;
  f.holes = (uint8_t)holes;
  f.filled = (uint8_t)__builtin_popcountll(board);
  f.flags = (uint8_t)((valid ? 4u : 1u) | (term ? 2u : 0u));
  f.last_blocks = (uint8_t)nblk;
  f.last_lines = (uint8_t)lines;
  f.last_cm = (uint8_t)cm;
  f.pad[0] = f.pad[1] = 0;
  return f;
}

}  // namespace bb
