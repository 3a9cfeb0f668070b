// bb_host.cpp -- host (CPU) backend of the env half of include/bbvec.h.
//
// A second implementation of the same C-ABI for machines without the MI355X,
// built by g++ into libbbvec_host.so (runtime/build.py build_host_lib).  It is
// selected explicitly (DeviceEnvBatch / VectorizedBlockBlastEnv with
// device="cpu"); nothing ever falls back to it: libbbvec.so still fails
// loudly without a HIP device, and the GPU tests never load this library.
// All "d_" pointers are host memory here and `stream` is ignored.
//
// Same semantics as the gfx950 kernels, bit for bit: uint64 bitboards (bit
// r*8+c), numpy-exact PCG64 piece streams, the reference's fp64 reward order,
// the vec-env auto-reset with its re-seed, the Philox synthetic policy.  The
// hand search is the reference DFS itself (engine.py:174-238) on bitboards, one
// env per thread (OpenMP over envs).  Parity: tests/test_host_backend.py runs it
// against the C oracle (oracle/bb_oracle.c) step for step.
//
// The hand word, the score of a move, the reward, the lookahead's value terms
// and the info record are the kernels' own definitions (bb_rules.h).  clear_full,
// anchors_of and the piece table are this file's plain loops on purpose: they
// are the independent check of the kernels' tuned versions.
//
// Reference: src/environment/wrappers.py:75-116 (vec step, auto-reset) ->
// block_blast_env.py:224-264 (step, reward 148-193) -> engine.py:390-454.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/bbvec.h"
#include "bb_look_rules.h"
#include "bb_rules.h"
#include "bb_seed.h"

namespace {

// the rules shared with the kernels (bb_rules.h), by name: nothing else of the header can meet this file's own
// clear_full, anchors_of, Pcg or Piece
using bb::kPieces, bb::kCol0, bb::kCenter;
using bb::hand_id, bb::hand_used, bb::hand_over, bb::hand_has32, bb::hand_pack, bb::hand_use, bb::hand_with_used,
    bb::hand_set_over;
using bb::count_holes, bb::combo_multiplier, bb::combo_next, bb::combo_after, bb::score_gained, bb::move_reward;
using bb::After, bb::after_reward, bb::pack_aux, bb::move_terms, bb::state_terms, bb::make_info;
using bb::seed::u128;

struct Piece {
  uint64_t shape, anchors;
  int n, off[9];
};

struct Tables {
  Piece p[kPieces];
  Tables() {
    for (int k = 0; k < kPieces; ++k) {
      Piece& q = p[k];
      q.shape = bb::seed::kShapes[k];
      q.n = 0;
      int h = 0, w = 0;
      for (int b = 0; b < 64; ++b)
        if ((q.shape >> b) & 1ull) {
          q.off[q.n++] = b;
          h = b / 8 + 1 > h ? b / 8 + 1 : h;
          w = b % 8 + 1 > w ? b % 8 + 1 : w;
        }
      q.anchors = 0;
      for (int r = 0; r <= 8 - h; ++r)
        for (int c = 0; c <= 8 - w; ++c) q.anchors |= 1ull << (r * 8 + c);
    }
  }
};
const Tables& T() {
  static const Tables t;
  return t;
}

// engine.py:364-380 / board.py:71-93 over all anchors: anchor a is blocked iff
// some cell a + off is filled
inline uint64_t anchors_of(int pid, uint64_t B) {
  const Piece& q = T().p[pid];
  uint64_t x = 0;
  for (int j = 0; j < q.n; ++j) x |= B >> q.off[j];
  return q.anchors & ~x;
}

// board.py:144-193: full rows / cols of the same board, union cleared
inline uint64_t clear_full(uint64_t B, int& rows, int& cols) {
  uint64_t rm = 0, cm = 0;
  rows = cols = 0;
  for (int r = 0; r < 8; ++r)
    if (((B >> (8 * r)) & 0xFFull) == 0xFFull) rm |= 0xFFull << (8 * r), ++rows;
  for (int c = 0; c < 8; ++c)
    if ((B & (kCol0 << c)) == (kCol0 << c)) cm |= kCol0 << c, ++cols;
  return B & ~(rm | cm);
}
inline uint64_t clear_full(uint64_t B) {
  int r, c;
  return clear_full(B, r, c);
}

// numpy PCG64 (XSL-RR) + Generator.integers(0, 37) buffered Lemire draw
struct Pcg {
  u128 state, inc;
  uint32_t buf;
  bool has;
};
inline uint64_t next64(Pcg& g) {
  g.state = g.state * bb::seed::kPcgMult + g.inc;
  const uint64_t hi = (uint64_t)(g.state >> 64), lo = (uint64_t)g.state;
  const uint64_t x = hi ^ lo;
  const unsigned rot = (unsigned)(hi >> 58);
  return (x >> rot) | (x << ((64u - rot) & 63u));
}
inline uint32_t next32(Pcg& g) {
  if (g.has) {
    g.has = false;
    return g.buf;
  }
  const uint64_t v = next64(g);
  g.has = true;
  g.buf = (uint32_t)(v >> 32);
  return (uint32_t)v;
}
inline uint32_t draw_piece(Pcg& g) {  // pieces.py:350-355, rng_excl 37: threshold (2^32 - 37) % 37 = 7
  uint64_t m = (uint64_t)next32(g) * 37ull;
  uint32_t left = (uint32_t)m;
  if (left < 37u)
    while (left < 7u) {
      m = (uint64_t)next32(g) * 37ull;
      left = (uint32_t)m;
    }
  return (uint32_t)(m >> 32);
}

// engine.py:174-238: can all three pieces be placed in some order, with the
// line clears in between?  (Only the boolean matters.)
bool solvable(uint64_t B, const uint32_t id[3]) {
  for (int f = 0; f < 3; ++f) {
    const int y = f == 0 ? 1 : 0, z = f == 2 ? 1 : 2;
    for (uint64_t a1 = anchors_of(id[f], B); a1; a1 &= a1 - 1) {
      const uint64_t B1 = clear_full(B | (T().p[id[f]].shape << __builtin_ctzll(a1)));
      for (int o = 0; o < 2; ++o) {
        const uint32_t py = id[o ? z : y], pz = id[o ? y : z];
        for (uint64_t a2 = anchors_of(py, B1); a2; a2 &= a2 - 1) {
          const uint64_t B2 = clear_full(B1 | (T().p[py].shape << __builtin_ctzll(a2)));
          if (anchors_of(pz, B2)) return true;
        }
      }
    }
  }
  return false;
}

// Philox4x32-10 word 0 at counter (idx, step) under key seed; the synthetic policy
uint32_t philox_w0(uint64_t seed, uint64_t idx, uint64_t step) {
  uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  return c0;
}
int32_t policy_action(const uint64_t m[3], uint32_t u) {
  const uint32_t tot = (uint32_t)(__builtin_popcountll(m[0]) + __builtin_popcountll(m[1]) + __builtin_popcountll(m[2]));
  if (tot == 0) return 0;
  uint32_t k = (uint32_t)(((uint64_t)u * tot) >> 32);
  for (int s = 0; s < 3; ++s) {
    const uint32_t c = (uint32_t)__builtin_popcountll(m[s]);
    if (k < c) {
      uint64_t x = m[s];
      for (uint32_t q = 0; q < k; ++q) x &= x - 1;
      return 64 * s + __builtin_ctzll(x);
    }
    k -= c;
  }
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------
// handle: structure-of-arrays state like the device slab (bb_device_ptrs)
// ---------------------------------------------------------------------------
struct bb_env {
  int n = 0;
  int autoreset = 1;
  bb_reward_cfg cfg{};
  std::vector<uint64_t> board, mask, seed_hi, seed_lo;
  std::vector<uint32_t> hand;  // packed hand word (bb_rules.h)
  std::vector<int64_t> score;
  std::vector<int32_t> combo, max_combo, moves, lines, blocks;
  std::vector<uint16_t> prev;  // _prev_holes | filled centre cells << 8
  std::vector<Pcg> rng;
  std::vector<uint8_t> has_seed;
  std::string err;
};

static thread_local std::string g_create_err;

namespace {

int fail(bb_env* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  else g_create_err = msg;
  return code;
}

// a lookahead call's broken argument rule (bb_look_rules.h) as BB_ERR_ARG with the text "<entry point>: <rule>";
// BB_OK (0) when no rule is broken
namespace R = bb_look_rules;
int refused(bb_env* e, const char* name, const char* rule) {
  return rule ? fail(e, BB_ERR_ARG, std::string(name) + ": " + rule) : BB_OK;
}

void masks_of(uint64_t B, uint32_t hand, uint64_t m[3]) {  // engine.py:364-380 (status not consulted)
  for (int s = 0; s < 3; ++s) m[s] = ((hand_used(hand) >> s) & 1u) ? 0ull : anchors_of(hand_id(hand, s), B);
}

// block_blast_env.py:195-222 -> engine.py:127-153: re-seed with seed_value when
// there is one, clear, first hand (every hand fits an empty board: no search)
void reset_env(bb_env* e, int i) {
  Pcg& g = e->rng[i];
  if (e->has_seed[i]) {
    g.state = ((u128)e->seed_hi[i] << 64) | e->seed_lo[i];
    g.buf = 0;
    g.has = false;
  }
  const uint32_t a = draw_piece(g), b = draw_piece(g), c = draw_piece(g);
  e->board[i] = 0;
  e->hand[i] = hand_pack(a, b, c, 0u, false, g.has);
  e->score[i] = 0;
  e->combo[i] = e->max_combo[i] = e->moves[i] = e->lines[i] = e->blocks[i] = 0;
  e->prev[i] = 0;  // _prev_holes = 0, _prev_center_openness = 1.0
  masks_of(0, e->hand[i], &e->mask[3 * (size_t)i]);
}

struct Out {
  double reward;
  bool term, valid;
  int lines;
};

// One env step (block_blast_env.py:224-264 with engine.make_move,
// engine.py:390-454) plus the vec env's auto-reset (wrappers.py:97-102).
Out step_env(bb_env* e, int i, int act, bb_info* info, int64_t* final_score, int32_t* final_moves) {
  Out o{-10.0, false, false, 0};  // invalid action (block_blast_env.py:240-245): no state change
  uint64_t B = e->board[i];
  uint32_t hand = e->hand[i];
  const int p = act >> 6, cell = act & 63;
  const uint32_t used = hand_used(hand);
  bool valid = act >= 0 && act < 192 && !hand_over(hand) && !((used >> p) & 1u);
  const Piece* pc = nullptr;
  if (valid) {
    pc = &T().p[hand_id(hand, p)];
    valid = ((pc->anchors >> cell) & 1ull) && ((pc->shape << cell) & B) == 0;
  }
  int nblk = 0, lines = 0, cm = 1, holes = 0;
  int64_t gained = 0;
  if (valid) {
    nblk = pc->n;
    e->moves[i] += 1;
    e->blocks[i] += nblk;
    int rows, cols;
    B = clear_full(B | (pc->shape << cell), rows, cols);
    lines = rows + cols;
    cm = combo_multiplier(lines);
    gained = score_gained(nblk, lines, combo_next(e->combo[i]));
    e->combo[i] = combo_after(lines, e->combo[i]);
    if (lines > 0 && e->combo[i] > e->max_combo[i]) e->max_combo[i] = e->combo[i];
    e->lines[i] += lines;
    e->score[i] += gained;
    const uint32_t nu = used | (1u << p);
    if (nu == 7u) {  // engine.py:432-437 -> _generate_new_pieces (155-172)
      Pcg& g = e->rng[i];
      uint32_t id[3] = {0, 0, 0};
      for (int attempt = 0; attempt < 100; ++attempt) {
        id[0] = draw_piece(g);
        id[1] = draw_piece(g);
        id[2] = draw_piece(g);
        if (solvable(B, id)) break;  // after 100 failures the last draw stays (engine.py:171-172)
      }
      hand = hand_pack(id[0], id[1], id[2], 0u, false, g.has);
    } else {
      hand = hand_with_used(hand, nu);
    }
    uint64_t m[3];
    masks_of(B, hand, m);
    const bool over = (m[0] | m[1] | m[2]) == 0ull;  // engine.py:440-441
    if (over) hand = hand_set_over(hand);
    holes = count_holes(B);
    const int center = __builtin_popcountll(B & kCenter);
    const double R = move_reward(e->cfg, e->cfg.center_bonus * 0.1, nblk, lines, cm, over, holes, center, e->prev[i]);
    e->prev[i] = (uint16_t)(holes | (center << 8));
    e->board[i] = B;
    e->hand[i] = hand;
    memcpy(&e->mask[3 * (size_t)i], m, sizeof(m));
    o = Out{R, over, true, lines};
  } else if (info) {
    holes = count_holes(B);
  }
  if (info)  // block_blast_env.py:266-288: after the move, before any auto-reset
    info[i] = make_info(e->score[i], gained, e->board[i], e->moves[i], e->lines[i], e->max_combo[i], e->blocks[i],
                        e->hand[i], holes, valid, o.term, nblk, lines, cm);
  if (o.term) {
    if (final_score) final_score[i] = e->score[i];
    if (final_moves) final_moves[i] = e->moves[i];
    if (e->autoreset) reset_env(e, i);
  }
  return o;
}

// ---------------------------------------------------------------------------
// one-ply lookahead (bbvec.h bb_afterstates / bb_greedy_actions): the host twin of csrc/bb_lookahead.hip
// ---------------------------------------------------------------------------
// engine.py:326-346 (legal), 390-431 (place, clear, combo, score) and the mobility of the slots that stay
// unused on the new board (engine.py:348-362)
After eval_action(uint64_t B, uint32_t hand, int combo, int act) {
  After a{};
  const int p = act >> 6, cell = act & 63;
  const uint32_t used0 = hand_used(hand), id = hand_id(hand, p);
  if (id >= (uint32_t)kPieces || hand_over(hand) || ((used0 >> p) & 1u)) return a;
  const Piece& pc = T().p[id];
  if (!((pc.anchors >> cell) & 1ull) || ((pc.shape << cell) & B)) return a;
  a.legal = true;
  a.ncells = pc.n;
  int rows, cols;
  a.board = clear_full(B | (pc.shape << cell), rows, cols);
  a.lines = rows + cols;
  a.combo1 = combo_after(a.lines, combo);
  a.gained = score_gained(a.ncells, a.lines, a.combo1);
  const uint32_t used = used0 | (1u << p);
  a.refill = used == 7u;
  for (int q = 0; q < 3; ++q)
    if (!((used >> q) & 1u) && hand_id(hand, q) < (uint32_t)kPieces)
      a.mobility += __builtin_popcountll(anchors_of((int)hand_id(hand, q), a.board));
  a.dead = !a.refill && a.mobility == 0;
  a.holes = count_holes(a.board);
  a.centre = __builtin_popcountll(a.board & kCenter);
  a.filled = __builtin_popcountll(a.board);
  return a;
}

void afterstates_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, const uint16_t* prev,
                      int32_t n, const bb_reward_cfg& cfg, const bb_afterstate_out& out) {
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; ++i) {
    const double center_tenth = cfg.center_bonus * 0.1;
    const uint32_t pv = prev ? prev[i] : 0u;
    for (int act = 0; act < 192; ++act) {
      const After a = eval_action(board[i], hand[i], combo ? combo[i] : 0, act);
      const size_t o = (size_t)i * 192 + (size_t)act;
      if (out.board) out.board[o] = a.legal ? a.board : board[i];
      if (out.reward_f64) out.reward_f64[o] = a.legal ? after_reward(a, cfg, center_tenth, pv) : -10.0;
      if (out.score_gained) out.score_gained[o] = a.legal ? (int32_t)a.gained : 0;
      if (out.aux) out.aux[o] = a.legal ? pack_aux(a) : 0u;
    }
  }
}

// `each`: w is the first of n rows and position i takes w[i] (the _each forms); else every position takes w[0]
void greedy_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int32_t n,
                 const bb_greedy_weights* rows, bool each, int32_t* action, int64_t* value) {
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; ++i) {
    const bb_greedy_weights& w = rows[each ? i : 0];
    int64_t best = INT64_MIN;
    int32_t best_a = 0;
    for (int act = 0; act < 192; ++act) {  // ascending: a later action must be strictly better
      const After a = eval_action(board[i], hand[i], combo ? combo[i] : 0, act);
      if (!a.legal) continue;
      const int64_t v = move_terms(w, a) + state_terms(w, a);
      if (v > best) best = v, best_a = act;
    }
    action[i] = best_a;
    if (value) value[i] = best;
  }
}

// ---------------------------------------------------------------------------
// full-hand lookahead (bbvec.h bb_plan_actions): the host twin of plan_kernel in csrc/bb_lookahead.hip, a
// plain depth-first search.  The actions are visited in ascending order at every ply and no maximal sequence
// is a prefix of another, so the leaves come in lexicographic order and a later one must be strictly better.
// ---------------------------------------------------------------------------
struct PlanBest {
  int64_t value;
  int32_t plan[3];
  int32_t leaves;
  bool alive;  // a maximal sequence ended in an afterstate that is not dead (bb_plan_values' safe)
};

template <class W>  // bb_greedy_weights, or bb_eval_weights (plan_ext_host): move_terms / state_terms of bb_rules.h
void plan_dfs(uint64_t B, uint32_t hand, int combo, int depth, int ply, int64_t sum, int32_t* seq, const W& w,
              PlanBest& best) {
  if (hand_over(hand)) return;  // game over: nothing is legal
  for (int p = 0; p < 3; ++p) {
    const uint32_t id = hand_id(hand, p);
    if (((hand_used(hand) >> p) & 1u) || id >= (uint32_t)kPieces) continue;
    for (uint64_t m = anchors_of((int)id, B); m; m &= m - 1) {
      const int act = p * 64 + __builtin_ctzll(m);
      const After a = eval_action(B, hand, combo, act);
      const int64_t s = sum + move_terms(w, a);
      seq[ply] = act;
      if (depth == 1 || a.refill || a.dead) {
        const int64_t v = s + state_terms(w, a);
        best.alive |= !a.dead;
        if (best.leaves++ == 0 || v > best.value) {
          best.value = v;
          for (int k = 0; k < 3; ++k) best.plan[k] = k <= ply ? seq[k] : -1;
        }
      } else {
        plan_dfs(a.board, hand_use(hand, p), a.combo1, depth - 1, ply + 1, s, seq, w, best);
      }
    }
  }
}

void plan_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int32_t n,
               const bb_greedy_weights* rows, bool each, int depth, const bb_plan_out& out) {  // rows: as greedy_host
#pragma omp parallel for schedule(dynamic, 1)  // the trees differ by orders of magnitude
  for (int32_t i = 0; i < n; ++i) {
    const bb_greedy_weights& w = rows[each ? i : 0];
    PlanBest best{INT64_MIN, {-1, -1, -1}, 0, false};
    int32_t seq[3];
    plan_dfs(board[i], hand[i], combo ? combo[i] : 0, depth, 0, 0, seq, w, best);
    out.action[i] = best.leaves ? best.plan[0] : 0;
    if (out.value) out.value[i] = best.value;
    if (out.plan)
      for (int k = 0; k < 3; ++k) out.plan[3 * (size_t)i + k] = best.plan[k];
    if (out.leaves) out.leaves[i] = best.leaves;
  }
}

// bbvec.h bb_plan_actions_ext (the host twin of plan_ext_kernel): the same DFS under a twelve-int row, whose state
// terms add the shape terms of the leaf's board; position i takes rows[i * w_stride], w_stride 0 or 1
void plan_ext_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int32_t n,
                   const bb_eval_weights* rows, int64_t w_stride, int depth, const bb_plan_out& out) {
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t i = 0; i < n; ++i) {
    const bb_eval_weights w = rows[(int64_t)i * w_stride];
    PlanBest best{INT64_MIN, {-1, -1, -1}, 0, false};
    int32_t seq[3];
    plan_dfs(board[i], hand[i], combo ? combo[i] : 0, depth, 0, 0, seq, w, best);
    out.action[i] = best.leaves ? best.plan[0] : 0;
    if (out.value) out.value[i] = best.value;
    if (out.plan)
      for (int k = 0; k < 3; ++k) out.plan[3 * (size_t)i + k] = best.plan[k];
    if (out.leaves) out.leaves[i] = best.leaves;
  }
}

// bbvec.h bb_board_terms: board_terms of bb_rules.h for every board
void board_terms_host(const uint64_t* board, int32_t n, int32_t* terms) {
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; ++i) bb::board_terms(board[i], &terms[4 * (size_t)i]);
}

// One position of bb_plan_values under either weight type: the same DFS, started below each first move
template <class W>
void plan_values_one(uint64_t board, uint32_t hand, int cb, size_t i, const W& w, int depth,
                     const bb_plan_values_out& out) {
  uint64_t safe[3] = {0, 0, 0};
  for (int act = 0; act < 192; ++act) {
    const After a = eval_action(board, hand, cb, act);
    PlanBest best{INT64_MIN, {-1, -1, -1}, 0, false};
    if (a.legal) {
      int32_t seq[3] = {act, -1, -1};
      if (depth == 1 || a.refill || a.dead) {
        best = PlanBest{move_terms(w, a) + state_terms(w, a), {act, -1, -1}, 1, !a.dead};
      } else {
        plan_dfs(a.board, hand_use(hand, act >> 6), a.combo1, depth - 1, 1, move_terms(w, a), seq, w, best);
      }
    }
    const size_t o = i * 192 + (size_t)act;
    if (out.q) out.q[o] = best.value;
    if (out.rest) out.rest[o] = a.legal ? (best.plan[1] & 0xFF) | ((best.plan[2] & 0xFF) << 8) : -1;
    if (out.leaves) out.leaves[o] = best.leaves;
    if (best.alive) safe[act >> 6] |= 1ull << (act & 63);
  }
  if (out.safe)
    for (int p = 0; p < 3; ++p) out.safe[3 * i + p] = safe[p];
}

// bbvec.h bb_plan_values (the host twin of plan_values_kernel)
void plan_values_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int32_t n,
                      const bb_greedy_weights& w, int depth, const bb_plan_values_out& out) {
  if (depth == 3 && !out.q && !out.rest && !out.leaves) depth = 2;  // the same safe set (bbvec.h)
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t i = 0; i < n; ++i) plan_values_one(board[i], hand[i], combo ? combo[i] : 0, (size_t)i, w, depth, out);
}

inline bool shaped(const bb_eval_weights& w) { return (w.perimeter | w.room3 | w.room5 | w.fits) != 0; }

// bbvec.h bb_plan_values_ext (the host twin of plan_values_ext_kernel): position i takes rows[i * w_stride], w_stride
// 0 or 1; a row with the four shape weights 0 is searched under its base, as the kernel does
void plan_values_ext_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int32_t n,
                          const bb_eval_weights* rows, int64_t w_stride, int depth, const bb_plan_values_out& out) {
  if (depth == 3 && !out.q && !out.rest && !out.leaves) depth = 2;  // the same safe set (bbvec.h)
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t i = 0; i < n; ++i) {
    const bb_eval_weights w = rows[(int64_t)i * w_stride];
    const int cb = combo ? combo[i] : 0;
    if (shaped(w))
      plan_values_one(board[i], hand[i], cb, (size_t)i, w, depth, out);
    else
      plan_values_one(board[i], hand[i], cb, (size_t)i, w.base, depth, out);
  }
}

// bbvec.h bb_safe_mask (the host twin of safe_mask_kernel): an existence search of its own on clear_full /
// anchors_of, not plan_dfs -- no values, no After.  Can the unused pieces of `hand` be placed on B in some order?
bool rest_fits(uint64_t B, uint32_t hand) {
  const uint32_t left = ~hand_used(hand) & 7u;
  if (!left) return true;  // the move before was a refill
  for (int q = 0; q < 3; ++q) {
    const uint32_t id = hand_id(hand, q);
    if (!((left >> q) & 1u) || id >= (uint32_t)kPieces) continue;
    for (uint64_t m = anchors_of((int)id, B); m; m &= m - 1)
      if (rest_fits(clear_full(B | (T().p[id].shape << __builtin_ctzll(m))), hand_use(hand, q))) return true;
  }
  return false;
}

void safe_mask_host(const uint64_t* board, const uint32_t* hand, int32_t n, int mode, uint64_t* mask) {
#pragma omp parallel for schedule(dynamic, 64)
  for (int32_t i = 0; i < n; ++i) {
    uint64_t safe[3] = {0, 0, 0}, legal[3] = {0, 0, 0};
    const uint64_t B = board[i];
    const uint32_t h = hand[i];
    for (int p = 0; p < 3 && !hand_over(h); ++p) {
      const uint32_t id = hand_id(h, p);
      if (((hand_used(h) >> p) & 1u) || id >= (uint32_t)kPieces) continue;
      legal[p] = anchors_of((int)id, B);
      for (uint64_t m = legal[p]; m; m &= m - 1) {
        const int cell = __builtin_ctzll(m);
        if (rest_fits(clear_full(B | (T().p[id].shape << cell)), hand_use(h, p))) safe[p] |= 1ull << cell;
      }
    }
    const bool keep = mode == BB_SAFE_WORDS || (safe[0] | safe[1] | safe[2]) != 0ull;
    for (int p = 0; p < 3; ++p) mask[3 * (size_t)i + p] = keep ? safe[p] : legal[p];
  }
}

// bbvec.h bb_refill_census (the host twin of census_kernel): which hands {a, b, c} engine.py:174-224 accepts on B.
// An existence search of its own on clear_full / anchors_of: for every first piece a and anchor x the afterstate B1,
// the anchors of all 37 pieces on B1 once, and the pairs {b, c} whose bit S[a][b] bit c is still clear; a's anchors
// end early once every pair is in.  S[a] is symmetric in (b, c); the hand's three choices of a first piece are
// joined at the end.
bool pair_fits(uint64_t X, int b, int c, const uint64_t A[kPieces]) {
  for (uint64_t m = A[b]; m; m &= m - 1)
    if (anchors_of(c, clear_full(X | (T().p[b].shape << __builtin_ctzll(m))))) return true;
  if (b != c)
    for (uint64_t m = A[c]; m; m &= m - 1)
      if (anchors_of(b, clear_full(X | (T().p[c].shape << __builtin_ctzll(m))))) return true;
  return false;
}

void refill_census_host(const uint64_t* board, int32_t n, const bb_census_out& out) {
  constexpr uint64_t kAll = (1ull << kPieces) - 1;
#pragma omp parallel for schedule(dynamic, 1)  // clogged and open boards differ by orders of magnitude
  for (int32_t i = 0; i < n; ++i) {
    const uint64_t B = board[i];
    uint64_t S[kPieces][kPieces] = {};
    for (int a = 0; a < kPieces; ++a) {
      int open = kPieces * (kPieces + 1) / 2;  // pairs b <= c not yet in S[a]
      for (uint64_t ma = anchors_of(a, B); ma && open; ma &= ma - 1) {
        const uint64_t B1 = clear_full(B | (T().p[a].shape << __builtin_ctzll(ma)));
        uint64_t A[kPieces];
        for (int p = 0; p < kPieces; ++p) A[p] = anchors_of(p, B1);
        for (int b = 0; b < kPieces; ++b) {
          if (S[a][b] == kAll) continue;
          for (int c = b; c < kPieces; ++c) {
            if (((S[a][b] >> c) & 1ull) || !(A[b] | A[c]) || !pair_fits(B1, b, c, A)) continue;
            S[a][b] |= 1ull << c;
            S[a][c] |= 1ull << b;
            --open;
          }
        }
      }
    }
    int32_t count = 0;
    for (int a = 0; a < kPieces; ++a)
      for (int b = 0; b < kPieces; ++b) {
        uint64_t w = S[a][b] | S[b][a];
        for (int c = 0; c < kPieces; ++c) w |= ((S[c][a] >> b) & 1ull) << c;
        if (out.solvable) out.solvable[((size_t)i * kPieces + a) * kPieces + b] = w;
        count += __builtin_popcountll(w);
      }
    if (out.count) out.count[i] = count;
  }
}

// Philox4x32-10 words 0..2 at counter (idx, step) under key seed: philox_w0's generator with the words kept
void philox_w012(uint64_t seed, uint64_t idx, uint64_t step, uint32_t out[3]) {
  uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
}

// The deal of pair (board B, stream idx, deal j): the dealer of engine.py:155-172 on Philox words with this file's own
// solvable().  Returns the hand; attempts is negative when nothing was accepted.  No weights are read.
uint32_t refill_deal(uint64_t B, uint64_t seed, uint64_t idx, int64_t j, int32_t& attempts) {
  uint32_t id[3] = {0, 0, 0};
  attempts = -100;
  for (int t = 0; t < 100; ++t) {
    uint32_t wd[3];
    philox_w012(seed, idx, ((uint64_t)j << 7) | (uint64_t)t, wd);
    for (int q = 0; q < 3; ++q) id[q] = (uint32_t)(((uint64_t)wd[q] * 37ull) >> 32);
    if (solvable(B, id)) {
      attempts = t + 1;
      break;  // after 100 refusals the last draw stays (engine.py:171-172)
    }
  }
  return hand_pack(id[0], id[1], id[2], 0u, false, false);
}

// plan_dfs on a dealt hand under either weight type; `dead` stands in when the hand has no legal first move
template <class W>
int64_t refill_search(uint64_t B, uint32_t hand, int combo, int depth, const W& w, int32_t dead) {
  PlanBest best{INT64_MIN, {-1, -1, -1}, 0, false};
  int32_t seq[3];
  plan_dfs(B, hand, combo, depth, 0, 0, seq, w, best);
  return best.leaves ? best.value : (int64_t)dead;
}

// bbvec.h bb_refill_values (the host twin of refill_values_kernel): the deal, then plan_dfs on the dealt hand.  One
// (board, deal) pair per iteration.
void refill_values_host(const uint64_t* board, const int32_t* combo, const uint64_t* stream_id, int32_t n,
                        const bb_greedy_weights& w, int depth, int32_t deals, uint64_t seed,
                        const bb_refill_values_out& out) {
  const int64_t pairs = (int64_t)n * deals;
#pragma omp parallel for schedule(dynamic, 1)  // the trees and the dealer loops differ by orders of magnitude
  for (int64_t k = 0; k < pairs; ++k) {
    const int64_t i = k / deals, j = k % deals;
    const uint64_t B = board[i], idx = stream_id ? stream_id[i] : (uint64_t)i;
    int32_t attempts;
    const uint32_t hand = refill_deal(B, seed, idx, j, attempts);
    if (out.hand) out.hand[k] = hand;
    if (out.attempts) out.attempts[k] = attempts;
    if (out.value) out.value[k] = refill_search(B, hand, combo ? combo[i] : 0, depth, w, w.dead);
  }
}

// bbvec.h bb_refill_values_ext (the host twin of refill_values_ext_kernel): every deal of board i is searched under
// rows[i * w_stride], w_stride 0 or 1; a hand without a legal first move gets the row's base.dead alone
void refill_values_ext_host(const uint64_t* board, const int32_t* combo, const uint64_t* stream_id, int32_t n,
                            const bb_eval_weights* rows, int64_t w_stride, int depth, int32_t deals, uint64_t seed,
                            const bb_refill_values_out& out) {
  const int64_t pairs = (int64_t)n * deals;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t k = 0; k < pairs; ++k) {
    const int64_t i = k / deals, j = k % deals;
    const uint64_t B = board[i], idx = stream_id ? stream_id[i] : (uint64_t)i;
    const bb_eval_weights w = rows[i * w_stride];
    int32_t attempts;
    const uint32_t hand = refill_deal(B, seed, idx, j, attempts);
    if (out.hand) out.hand[k] = hand;
    if (out.attempts) out.attempts[k] = attempts;
    if (out.value) {
      const int cb = combo ? combo[i] : 0;
      out.value[k] = shaped(w) ? refill_search(B, hand, cb, depth, w, w.base.dead)
                               : refill_search(B, hand, cb, depth, w.base, w.base.dead);
    }
  }
}

// One plan played to its leaf (bbvec.h bb_play_plan_pos): the state reached, the lines and score summed, the status word
struct Leaf {
  uint64_t board;
  uint32_t hand;
  int combo;
  int32_t lines;
  int64_t score;
  uint32_t status;
};
Leaf play_plan_one(uint64_t B, uint32_t h, int cb, const int32_t* plan) {
  Leaf f{B, h, cb, 0, 0, 0u};
  for (int k = 0; k < 3; ++k) {
    const int32_t act = plan[k];
    if (act < 0) break;  // a ply not played
    const After a = act < 192 ? eval_action(f.board, f.hand, f.combo, act) : After{};
    if (!a.legal) {
      f.status |= BB_PLAY_ILLEGAL;
      break;
    }
    f.board = a.board;
    f.hand = hand_use(f.hand, act >> 6);
    f.combo = a.combo1;
    f.lines += a.lines;
    f.score += a.gained;
    f.status = (uint32_t)(k + 1) | (a.dead ? BB_PLAY_DEAD : 0u) | (a.refill ? BB_PLAY_REFILL : 0u);
  }
  return f;
}

// bbvec.h bb_play_plan_pos (the host twin of play_plan_kernel)
void play_plan_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int32_t n, const int32_t* plan,
                    const bb_play_plan_out& out) {
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; ++i) {
    const Leaf f = play_plan_one(board[i], hand[i], combo ? combo[i] : 0, &plan[3 * (size_t)i]);
    if (out.board) out.board[i] = f.board;
    if (out.hand) out.hand[i] = f.hand;
    if (out.combo) out.combo[i] = f.combo;
    if (out.lines) out.lines[i] = f.lines;
    if (out.score) out.score[i] = f.score;
    if (out.status) out.status[i] = (int32_t)f.status;
  }
}

// bbvec.h bb_plan2_values (the host twin of plan_values_ext_kernel and the three plan2 kernels): steps 1-3 over the
// roots, step 4 over the (root, candidate, deal) triples, steps 5-6 over the roots.  Everything in between lives in the
// caller's workspace, carved as the HIP backend carves it (bb_look_rules.h Plan2Layout); nothing is allocated.
void plan2_values_host(const uint64_t* board, const uint32_t* hand, const int32_t* combo, const uint64_t* stream_id,
                       int32_t n, const bb_eval_weights* rows, int64_t w_stride, int depth, int32_t K, int32_t deals,
                       uint64_t seed, void* work, const bb_plan2_out& out) {
  const R::Plan2Layout lay(n, K, deals);
  char* base = static_cast<char*>(work);
  int64_t* q = reinterpret_cast<int64_t*>(base + lay.q);
  uint64_t* leaf_board = reinterpret_cast<uint64_t*>(base + lay.board);
  int64_t* moved = reinterpret_cast<int64_t*>(base + lay.moved);
  int64_t* value = out.value ? out.value : reinterpret_cast<int64_t*>(base + lay.value);
  int32_t* rest = reinterpret_cast<int32_t*>(base + lay.rest);
  int32_t* leaf_combo = reinterpret_cast<int32_t*>(base + lay.combo);
  int32_t* cand = out.cand ? out.cand : reinterpret_cast<int32_t*>(base + lay.cand);
  int32_t* status = out.status ? out.status : reinterpret_cast<int32_t*>(base + lay.status);
  const bb_plan_values_out pv{q, rest, nullptr, nullptr};

  // ---- steps 1-3: the values, the candidates by rank, their leaves
#pragma omp parallel for schedule(dynamic, 1)
  for (int32_t i = 0; i < n; ++i) {
    const bb_eval_weights w = rows[(int64_t)i * w_stride];
    const int cb = combo ? combo[i] : 0;
    if (shaped(w))
      plan_values_one(board[i], hand[i], cb, (size_t)i, w, depth, pv);
    else
      plan_values_one(board[i], hand[i], cb, (size_t)i, w.base, depth, pv);
    const int64_t* qi = q + (size_t)i * 192;
    const int32_t* ri = rest + (size_t)i * 192;
    int32_t legal = 0;
    for (int a = 0; a < 192; ++a) {
      if (qi[a] == INT64_MIN) continue;  // never a candidate
      ++legal;
      int32_t rank = 0;  // the place of a in a stable descending sort
      for (int b = 0; b < 192; ++b) rank += qi[b] > qi[a] || (qi[b] == qi[a] && b < a);
      if (rank >= K) continue;
      const int r2 = ri[a] & 0xFF, r3 = (ri[a] >> 8) & 0xFF;
      const int32_t plan[3] = {a, r2 == 0xFF ? -1 : r2, r3 == 0xFF ? -1 : r3};
      const Leaf f = play_plan_one(board[i], hand[i], cb, plan);
      const size_t c = (size_t)i * K + (size_t)rank;
      cand[c] = a;
      leaf_board[c] = f.board;
      leaf_combo[c] = f.combo;
      moved[c] = (int64_t)w.base.lines * f.lines + (int64_t)w.base.score * f.score;
      status[c] = (int32_t)f.status;
    }
    for (int32_t r = legal; r < K; ++r) cand[(size_t)i * K + r] = status[(size_t)i * K + r] = -1;
  }

  // ---- step 4: one (root, candidate, deal) triple per iteration, under the root's row and stream id
  const int64_t triples = (int64_t)n * K * deals;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t t = 0; t < triples; ++t) {
    const int64_t c = t / deals, j = t % deals, i = c / K;
    if (status[c] < 0 || !((uint32_t)status[c] & BB_PLAY_REFILL)) {
      value[t] = 0;
      continue;
    }
    const bb_eval_weights w = rows[i * w_stride];
    int32_t attempts;
    const uint32_t dealt = refill_deal(leaf_board[c], seed, stream_id ? stream_id[i] : (uint64_t)i, j, attempts);
    value[t] = shaped(w) ? refill_search(leaf_board[c], dealt, leaf_combo[c], depth, w, w.base.dead)
                         : refill_search(leaf_board[c], dealt, leaf_combo[c], depth, w.base, w.base.dead);
  }

  // ---- steps 5-6: Q2 and the choice, ties to the lower action
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; ++i) {
    int64_t* q2 = out.q2 ? out.q2 + (size_t)i * 192 : nullptr;
    if (q2)
      for (int a = 0; a < 192; ++a) q2[a] = INT64_MIN;
    int64_t best = INT64_MIN;
    int32_t best_a = 192;
    for (int32_t r = 0; r < K; ++r) {
      const size_t c = (size_t)i * K + (size_t)r;
      const int32_t a = cand[c];
      if (a < 0) continue;
      int64_t x;
      if ((uint32_t)status[c] & BB_PLAY_REFILL) {
        x = (int64_t)deals * moved[c];
        for (int32_t j = 0; j < deals; ++j) x += value[c * deals + (size_t)j];
      } else {
        x = (int64_t)deals * q[(size_t)i * 192 + (size_t)a];
      }
      if (q2) q2[a] = x;
      if (x > best || (x == best && a < best_a)) best = x, best_a = a;
    }
    if (out.action) out.action[i] = best_a == 192 ? 0 : best_a;
  }
}

// bbvec.h bb_playout_values (the host twin of playout_values_kernel): one (board, playout) pair per iteration; per hand
// refill_deal under key seed + h, plan_dfs on the dealt hand (bb_plan_actions_ext's search) and play_plan_one on the
// plan found, the board and the combo carried.
template <class W>
PlanBest playout_search(uint64_t B, uint32_t hand, int combo, int depth, const W& w) {
  PlanBest best{INT64_MIN, {-1, -1, -1}, 0, false};
  int32_t seq[3];
  plan_dfs(B, hand, combo, depth, 0, 0, seq, w, best);
  return best;
}

void playout_values_host(const uint64_t* board, const int32_t* combo, const uint64_t* stream_id, int32_t n,
                         const bb_eval_weights* rows, int64_t w_stride, int depth, int32_t playouts, int32_t hands,
                         uint64_t seed, const bb_playout_out& out) {
  const int64_t pairs = (int64_t)n * playouts;
#pragma omp parallel for schedule(dynamic, 1)  // the playouts end after different numbers of hands
  for (int64_t k = 0; k < pairs; ++k) {
    const int64_t i = k / playouts, j = k % playouts;
    const uint64_t idx = stream_id ? stream_id[i] : (uint64_t)i;
    const bb_eval_weights w = rows[i * w_stride];
    uint64_t B = board[i];
    int cb = combo ? combo[i] : 0;
    int64_t moved = 0, score = 0, value = 0;
    int32_t lines = 0, plies = 0, searched = 0;
    uint32_t dealt = 0u, status = 0u;
    for (int32_t h = 0; h < hands; ++h) {
      int32_t attempts;
      dealt = refill_deal(B, seed + (uint64_t)h, idx, j, attempts);
      const PlanBest best = shaped(w) ? playout_search(B, dealt, cb, depth, w) : playout_search(B, dealt, cb, depth, w.base);
      searched = h + 1;
      if (!best.leaves) {  // no legal first move: nothing is played
        value = moved + (int64_t)w.base.dead;
        status = 0u;
        break;
      }
      value = moved + best.value;
      const Leaf f = play_plan_one(B, dealt, cb, best.plan);
      B = f.board;
      cb = f.combo;
      lines += f.lines;
      score += f.score;
      plies += (int32_t)(f.status & BB_PLAY_PLIES);
      status = f.status;
      if (!(status & BB_PLAY_REFILL)) break;  // a dead leaf, or a plan cut short by depth < 3
      moved += (int64_t)w.base.lines * f.lines + (int64_t)w.base.score * f.score;
    }
    if (out.value) out.value[k] = value;
    if (out.score) out.score[k] = score;
    if (out.lines) out.lines[k] = lines;
    if (out.plies) out.plies[k] = plies;
    if (out.hands) out.hands[k] = searched;
    if (out.status) out.status[k] = (int32_t)status;
    if (out.board) out.board[k] = B;
    if (out.combo) out.combo[k] = cb;
    if (out.hand) out.hand[k] = dealt;
  }
}

}  // namespace

#ifndef BB_BUILD_ID
#define BB_BUILD_ID "unhashed"
#endif
static const char kBuildIdMarker[] = "bbvec-build-id:" BB_BUILD_ID;  // runtime/build.py host_source_id

extern "C" {

int bb_abi_version(void) { return BB_ABI_VERSION; }

const char* bb_build_id(void) { return kBuildIdMarker + 15; }

const char* bb_last_error(const bb_env* env) { return env ? env->err.c_str() : g_create_err.c_str(); }

int32_t bb_num_envs(const bb_env* env) { return env ? env->n : 0; }

int bb_pcg64_seed(uint64_t seed, uint64_t out[4]) {
  if (!out) return BB_ERR_ARG;
  bb::seed::pcg64_seed_numpy(seed, out);
  return BB_OK;
}

int bb_create(int32_t num_envs, int32_t device, const bb_reward_cfg* cfg, int32_t autoreset, bb_env** out) {
  (void)device;  // the host backend has no devices
  if (!out) return fail(nullptr, BB_ERR_ARG, "bb_create: out is NULL");
  *out = nullptr;
  if (num_envs <= 0) return fail(nullptr, BB_ERR_ARG, "bb_create: num_envs must be positive");
  if (!cfg) return fail(nullptr, BB_ERR_ARG, "bb_create: reward config is NULL");
  bb_env* e = new bb_env();
  const size_t n = (size_t)num_envs;
  e->n = num_envs;
  e->autoreset = autoreset ? 1 : 0;
  e->cfg = *cfg;
  e->board.assign(n, 0);
  e->mask.assign(3 * n, 0);
  e->seed_hi.assign(n, 0);
  e->seed_lo.assign(n, 0);
  e->hand.assign(n, 0);
  e->score.assign(n, 0);
  e->combo.assign(n, 0);
  e->max_combo.assign(n, 0);
  e->moves.assign(n, 0);
  e->lines.assign(n, 0);
  e->blocks.assign(n, 0);
  e->prev.assign(n, 0);
  e->rng.assign(n, Pcg{0, 1, 0, false});
  e->has_seed.assign(n, 0);
  *out = e;
  return BB_OK;
}

void bb_destroy(bb_env* env) { delete env; }

int bb_seed(bb_env* env, const uint64_t* h_seeds, const uint8_t* h_has_seed, const uint64_t* h_raw) {
  if (!env) return BB_ERR_ARG;
  if (!h_has_seed) return fail(env, BB_ERR_ARG, "bb_seed: has_seed is NULL");
  for (int i = 0; i < env->n; ++i) {
    uint64_t w[4];
    if (h_has_seed[i] == 1) {
      if (!h_seeds) return fail(env, BB_ERR_ARG, "bb_seed: seeds is NULL");
      bb::seed::pcg64_seed_numpy(h_seeds[i], w);
    } else {
      if (!h_raw) return fail(env, BB_ERR_ARG, "bb_seed: raw state is NULL");
      for (int k = 0; k < 4; ++k) w[k] = h_raw[4 * (size_t)i + k];
      w[3] |= 1ull;  // PCG increments are odd
    }
    env->has_seed[i] = h_has_seed[i] ? 1 : 0;
    env->seed_hi[i] = w[0];
    env->seed_lo[i] = w[1];
    env->rng[i] = Pcg{((u128)w[0] << 64) | w[1], ((u128)w[2] << 64) | w[3], 0, false};
    env->hand[i] = 0;
  }
  return BB_OK;
}

int bb_reset(bb_env* env, const uint8_t* d_env_mask, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
#pragma omp parallel for schedule(static)
  for (int i = 0; i < env->n; ++i) {
    if (d_env_mask && !d_env_mask[i]) continue;
    env->rng[i].has = hand_has32(env->hand[i]);
    reset_env(env, i);
  }
  return BB_OK;
}

int bb_step(bb_env* env, const int32_t* d_actions, const bb_step_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (!d_actions || !out || !out->reward || !out->terminated)
    return fail(env, BB_ERR_ARG, "bb_step: actions, reward and terminated are required");
#pragma omp parallel for schedule(dynamic, 256)
  for (int i = 0; i < env->n; ++i) {
    const Out o = step_env(env, i, d_actions[i], out->info, out->final_score, out->final_moves);
    out->reward[i] = (float)o.reward;
    out->terminated[i] = o.term ? 1 : 0;
    if (out->reward_f64) out->reward_f64[i] = o.reward;
    if (out->lines) out->lines[i] = (uint8_t)o.lines;
    const uint64_t* m = &env->mask[3 * (size_t)i];
    if (out->mask) memcpy(&out->mask[3 * (size_t)i], m, 24);
    if (out->next_action)
      out->next_action[i] = policy_action(m, philox_w0(out->policy_seed, out->env_offset + (uint64_t)i, out->policy_step));
  }
  return BB_OK;
}

int bb_rollout(bb_env* env, int32_t steps, const int32_t* d_actions, const bb_rollout_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (steps < 0) return fail(env, BB_ERR_ARG, "bb_rollout: steps must be >= 0");
  if (!d_actions || !out || !out->reward || !out->terminated)
    return fail(env, BB_ERR_ARG, "bb_rollout: actions, reward and terminated are required");
  const size_t n = (size_t)env->n;
#pragma omp parallel for schedule(dynamic, 64)
  for (int i = 0; i < env->n; ++i) {
    int32_t a = d_actions[i];
    for (int t = 0; t < steps; ++t) {
      const Out o = step_env(env, i, a, nullptr, nullptr, nullptr);
      const size_t k = (size_t)t * n + (size_t)i;
      out->reward[k] = (float)o.reward;
      out->terminated[k] = o.term ? 1 : 0;
      if (out->lines) out->lines[k] = (uint8_t)o.lines;
      if (out->actions) out->actions[k] = a;
      const uint64_t* m = &env->mask[3 * (size_t)i];
      if (out->mask) memcpy(&out->mask[3 * k], m, 24);
      a = policy_action(m, philox_w0(out->policy_seed, out->env_offset + (uint64_t)i,
                                     out->policy_step0 + (uint64_t)t + 1));
    }
    if (out->next_action && steps > 0) out->next_action[i] = a;
  }
  return BB_OK;
}

// every call runs to completion on the calling thread, and no loop here is bounded by a cap: nothing to report
int bb_sync(bb_env* env, void* stream) {
  (void)stream;
  return env ? BB_OK : BB_ERR_ARG;
}

// engine.py:478-507 / wrappers.py:118-126: board plane + unused pieces' shapes at
// the origin, f32 [N][4][8][8]; masks as int8 / f32 [N][192] and bits [N][3]
int bb_obs(bb_env* env, float* d_x, int8_t* d_mask_i8, float* d_mask_f32, uint64_t* d_mask_bits, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
#pragma omp parallel for schedule(static)
  for (int i = 0; i < env->n; ++i) {
    const uint64_t* m = &env->mask[3 * (size_t)i];
    if (d_x) {
      float* x = d_x + (size_t)i * 256;
      const uint32_t h = env->hand[i];
      for (int pl = 0; pl < 4; ++pl) {
        const uint64_t v = pl == 0 ? env->board[i]
                                   : (((hand_used(h) >> (pl - 1)) & 1u) ? 0ull : T().p[hand_id(h, pl - 1)].shape);
        for (int b = 0; b < 64; ++b) x[64 * pl + b] = (float)((v >> b) & 1ull);
      }
    }
    for (int a = 0; a < 192; ++a) {
      const int bit = (int)((m[a >> 6] >> (a & 63)) & 1ull);
      if (d_mask_i8) d_mask_i8[(size_t)i * 192 + a] = (int8_t)bit;
      if (d_mask_f32) d_mask_f32[(size_t)i * 192 + a] = (float)bit;
    }
    if (d_mask_bits) memcpy(&d_mask_bits[3 * (size_t)i], m, 24);
  }
  return BB_OK;
}

int bb_device_ptrs(bb_env* env, uint64_t** d_board, uint32_t** d_hand, uint64_t** d_mask) {
  if (!env) return BB_ERR_ARG;
  if (d_board) *d_board = env->board.data();
  if (d_hand) *d_hand = env->hand.data();
  if (d_mask) *d_mask = env->mask.data();
  return BB_OK;
}

int bb_snapshot(bb_env* env, uint64_t* d_board, uint32_t* d_hand, uint64_t* d_mask_bits, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  const size_t n = (size_t)env->n;
  if (d_board) memcpy(d_board, env->board.data(), n * 8);
  if (d_hand) memcpy(d_hand, env->hand.data(), n * 4);
  if (d_mask_bits) memcpy(d_mask_bits, env->mask.data(), n * 24);
  return BB_OK;
}

int bb_snapshot_combo(bb_env* env, int32_t* d_combo, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (d_combo) memcpy(d_combo, env->combo.data(), (size_t)env->n * 4);
  return BB_OK;
}

int bb_get_state(bb_env* env, const bb_state_view* v) {
  if (!env || !v) return BB_ERR_ARG;
  const size_t n = (size_t)env->n;
  if (v->board) memcpy(v->board, env->board.data(), n * 8);
  if (v->hand) memcpy(v->hand, env->hand.data(), n * 4);
  if (v->score) memcpy(v->score, env->score.data(), n * 8);
  if (v->combo) memcpy(v->combo, env->combo.data(), n * 4);
  if (v->max_combo) memcpy(v->max_combo, env->max_combo.data(), n * 4);
  if (v->moves) memcpy(v->moves, env->moves.data(), n * 4);
  if (v->lines) memcpy(v->lines, env->lines.data(), n * 4);
  if (v->blocks) memcpy(v->blocks, env->blocks.data(), n * 4);
  for (size_t i = 0; i < n; ++i) {
    if (v->prev_holes) v->prev_holes[i] = (uint8_t)(env->prev[i] & 0xFF);
    if (v->prev_center) v->prev_center[i] = (uint8_t)(env->prev[i] >> 8);
    if (v->rng) {
      v->rng[3 * i] = (uint64_t)(env->rng[i].state >> 64);
      v->rng[3 * i + 1] = (uint64_t)env->rng[i].state;
      v->rng[3 * i + 2] = env->rng[i].buf;
    }
  }
  return BB_OK;
}

int bb_set_state(bb_env* env, const bb_state_view* v) {
  if (!env || !v) return BB_ERR_ARG;
  const size_t n = (size_t)env->n;
  if (v->board) memcpy(env->board.data(), v->board, n * 8);
  if (v->hand) memcpy(env->hand.data(), v->hand, n * 4);
  if (v->score) memcpy(env->score.data(), v->score, n * 8);
  if (v->combo) memcpy(env->combo.data(), v->combo, n * 4);
  if (v->max_combo) memcpy(env->max_combo.data(), v->max_combo, n * 4);
  if (v->moves) memcpy(env->moves.data(), v->moves, n * 4);
  if (v->lines) memcpy(env->lines.data(), v->lines, n * 4);
  if (v->blocks) memcpy(env->blocks.data(), v->blocks, n * 4);
  for (size_t i = 0; i < n; ++i) {
    const uint16_t h = v->prev_holes ? v->prev_holes[i] : (uint16_t)(env->prev[i] & 0xFF);
    const uint16_t c = v->prev_center ? v->prev_center[i] : (uint16_t)(env->prev[i] >> 8);
    env->prev[i] = (uint16_t)(h | (c << 8));
    if (v->rng) {
      env->rng[i].state = ((u128)v->rng[3 * i] << 64) | v->rng[3 * i + 1];
      env->rng[i].buf = (uint32_t)v->rng[3 * i + 2];
    }
    env->rng[i].has = hand_has32(env->hand[i]);
    masks_of(env->board[i], env->hand[i], &env->mask[3 * i]);  // derived state
  }
  return BB_OK;
}

int bb_random_actions(const uint64_t* d_mask_bits, int32_t n, uint64_t seed, uint64_t step, uint64_t env_offset,
                      int32_t* d_actions, void* stream) {
  (void)stream;
  if (!d_mask_bits || !d_actions || n < 0) return fail(nullptr, BB_ERR_ARG, "bb_random_actions: bad arguments");
  for (int32_t i = 0; i < n; ++i)
    d_actions[i] = policy_action(&d_mask_bits[3 * (size_t)i], philox_w0(seed, env_offset + (uint64_t)i, step));
  return BB_OK;
}

// Lookahead.  The argument rules are those of csrc/bb_capi.cpp, from the same header (bb_look_rules.h).

int bb_afterstates_pos(const bb_positions* pos, int32_t n, const bb_reward_cfg* cfg, const bb_afterstate_out* out,
                       void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_afterstates_pos", R::afterstates_pos(pos, n, cfg, out))) return rc;
  afterstates_host(pos->board, pos->hand, pos->combo, pos->prev, n, *cfg, *out);
  return BB_OK;
}

int bb_afterstates(bb_env* env, const bb_afterstate_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_afterstates", R::afterstates(out))) return rc;
  afterstates_host(env->board.data(), env->hand.data(), env->combo.data(), env->prev.data(), env->n, env->cfg, *out);
  return BB_OK;
}

int bb_greedy_actions_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t* d_action,
                          int64_t* d_value, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_greedy_actions_pos", R::greedy_actions_pos(pos, n, w, d_action))) return rc;
  greedy_host(pos->board, pos->hand, pos->combo, n, w, false, d_action, d_value);
  return BB_OK;
}

int bb_greedy_actions(bb_env* env, const bb_greedy_weights* w, int32_t* d_action, int64_t* d_value, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_greedy_actions", R::greedy_actions(w, d_action))) return rc;
  greedy_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, w, false, d_action, d_value);
  return BB_OK;
}

int bb_plan_actions_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t depth,
                        const bb_plan_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_plan_actions_pos", R::plan_actions_pos(pos, n, w, depth, out))) return rc;
  plan_host(pos->board, pos->hand, pos->combo, n, w, false, depth, *out);
  return BB_OK;
}

int bb_plan_actions(bb_env* env, const bb_greedy_weights* w, int32_t depth, const bb_plan_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_plan_actions", R::plan_actions(w, depth, out))) return rc;
  plan_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, w, false, depth, *out);
  return BB_OK;
}

// One row of weights per position: d_w is host memory here, [n] ([num_envs]) rows

int bb_greedy_actions_each_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* d_w, int32_t* d_action,
                               int64_t* d_value, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_greedy_actions_each_pos", R::greedy_actions_each_pos(pos, n, d_w, d_action)))
    return rc;
  greedy_host(pos->board, pos->hand, pos->combo, n, d_w, true, d_action, d_value);
  return BB_OK;
}

int bb_greedy_actions_each(bb_env* env, const bb_greedy_weights* d_w, int32_t* d_action, int64_t* d_value,
                           void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_greedy_actions_each", R::greedy_actions_each(d_w, d_action))) return rc;
  greedy_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, d_w, true, d_action, d_value);
  return BB_OK;
}

int bb_plan_actions_each_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* d_w, int32_t depth,
                             const bb_plan_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_plan_actions_each_pos", R::plan_actions_each_pos(pos, n, d_w, depth, out)))
    return rc;
  plan_host(pos->board, pos->hand, pos->combo, n, d_w, true, depth, *out);
  return BB_OK;
}

int bb_plan_actions_each(bb_env* env, const bb_greedy_weights* d_w, int32_t depth, const bb_plan_out* out,
                         void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_plan_actions_each", R::plan_actions_each(d_w, depth, out))) return rc;
  plan_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, d_w, true, depth, *out);
  return BB_OK;
}

// The shape terms and the search with them: d_w is host memory here

int bb_board_terms_pos(const uint64_t* d_board, int32_t n, int32_t* d_terms, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_board_terms_pos", R::board_terms_pos(d_board, n, d_terms))) return rc;
  board_terms_host(d_board, n, d_terms);
  return BB_OK;
}

int bb_board_terms(bb_env* env, int32_t* d_terms, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_board_terms", R::board_terms(d_terms))) return rc;
  board_terms_host(env->board.data(), env->n, d_terms);
  return BB_OK;
}

int bb_plan_actions_ext_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w, int64_t w_stride,
                            int32_t depth, const bb_plan_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_plan_actions_ext_pos", R::plan_actions_ext_pos(pos, n, d_w, w_stride, depth, out)))
    return rc;
  plan_ext_host(pos->board, pos->hand, pos->combo, n, d_w, w_stride, depth, *out);
  return BB_OK;
}

int bb_plan_actions_ext(bb_env* env, const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                        const bb_plan_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_plan_actions_ext", R::plan_actions_ext(d_w, w_stride, depth, out))) return rc;
  plan_ext_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, d_w, w_stride, depth, *out);
  return BB_OK;
}

int bb_plan_values_pos(const bb_positions* pos, int32_t n, const bb_greedy_weights* w, int32_t depth,
                       const bb_plan_values_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_plan_values_pos", R::plan_values_pos(pos, n, w, depth, out))) return rc;
  plan_values_host(pos->board, pos->hand, pos->combo, n, *w, depth, *out);
  return BB_OK;
}

int bb_plan_values(bb_env* env, const bb_greedy_weights* w, int32_t depth, const bb_plan_values_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_plan_values", R::plan_values(w, depth, out))) return rc;
  plan_values_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, *w, depth, *out);
  return BB_OK;
}

int bb_safe_mask_pos(const bb_positions* pos, int32_t n, int32_t mode, uint64_t* d_mask, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_safe_mask_pos", R::safe_mask_pos(pos, n, mode, d_mask))) return rc;
  safe_mask_host(pos->board, pos->hand, n, mode, d_mask);
  return BB_OK;
}

int bb_safe_mask(bb_env* env, int32_t mode, uint64_t* d_mask, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_safe_mask", R::safe_mask(mode, d_mask))) return rc;
  safe_mask_host(env->board.data(), env->hand.data(), env->n, mode, d_mask);
  return BB_OK;
}

int bb_refill_census_pos(const uint64_t* d_board, int32_t n, const bb_census_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_refill_census_pos", R::refill_census_pos(d_board, n, out))) return rc;
  refill_census_host(d_board, n, *out);
  return BB_OK;
}

int bb_refill_census(bb_env* env, const bb_census_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_refill_census", R::refill_census(out))) return rc;
  refill_census_host(env->board.data(), env->n, *out);
  return BB_OK;
}

int bb_refill_values_pos(const uint64_t* d_board, const int32_t* d_combo, const uint64_t* d_stream, int32_t n,
                         const bb_greedy_weights* w, int32_t depth, int32_t deals, uint64_t seed,
                         const bb_refill_values_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_refill_values_pos", R::refill_values_pos(d_board, n, w, depth, deals, out)))
    return rc;
  refill_values_host(d_board, d_combo, d_stream, n, *w, depth, deals, seed, *out);
  return BB_OK;
}

int bb_refill_values(bb_env* env, const uint64_t* d_stream, const bb_greedy_weights* w, int32_t depth, int32_t deals,
                     uint64_t seed, const bb_refill_values_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_refill_values", R::refill_values(w, depth, deals, out))) return rc;
  refill_values_host(env->board.data(), env->combo.data(), d_stream, env->n, *w, depth, deals, seed, *out);
  return BB_OK;
}

int bb_plan_values_ext_pos(const bb_positions* pos, int32_t n, const bb_eval_weights* d_w, int64_t w_stride,
                           int32_t depth, const bb_plan_values_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_plan_values_ext_pos", R::plan_values_ext_pos(pos, n, d_w, w_stride, depth, out)))
    return rc;
  plan_values_ext_host(pos->board, pos->hand, pos->combo, n, d_w, w_stride, depth, *out);
  return BB_OK;
}

int bb_plan_values_ext(bb_env* env, const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                       const bb_plan_values_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_plan_values_ext", R::plan_values_ext(d_w, w_stride, depth, out))) return rc;
  plan_values_ext_host(env->board.data(), env->hand.data(), env->combo.data(), env->n, d_w, w_stride, depth, *out);
  return BB_OK;
}

int bb_refill_values_ext_pos(const uint64_t* d_board, const int32_t* d_combo, const uint64_t* d_stream, int32_t n,
                             const bb_eval_weights* d_w, int64_t w_stride, int32_t depth, int32_t deals,
                             uint64_t seed, const bb_refill_values_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_refill_values_ext_pos",
                       R::refill_values_ext_pos(d_board, n, d_w, w_stride, depth, deals, out)))
    return rc;
  refill_values_ext_host(d_board, d_combo, d_stream, n, d_w, w_stride, depth, deals, seed, *out);
  return BB_OK;
}

int bb_refill_values_ext(bb_env* env, const uint64_t* d_stream, const bb_eval_weights* d_w, int64_t w_stride,
                         int32_t depth, int32_t deals, uint64_t seed, const bb_refill_values_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_refill_values_ext", R::refill_values_ext(d_w, w_stride, depth, deals, out))) return rc;
  refill_values_ext_host(env->board.data(), env->combo.data(), d_stream, env->n, d_w, w_stride, depth, deals, seed,
                         *out);
  return BB_OK;
}

int bb_play_plan_pos(const bb_positions* pos, int32_t n, const int32_t* d_plan, const bb_play_plan_out* out,
                     void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_play_plan_pos", R::play_plan_pos(pos, n, d_plan, out))) return rc;
  play_plan_host(pos->board, pos->hand, pos->combo, n, d_plan, *out);
  return BB_OK;
}

int64_t bb_plan2_work_bytes(int32_t n, int32_t candidates, int32_t deals) {
  return R::plan2_work_bytes(n, candidates, deals);
}

int bb_plan2_values_pos(const bb_positions* pos, const uint64_t* d_stream, int32_t n, const bb_eval_weights* d_w,
                        int64_t w_stride, int32_t depth, int32_t candidates, int32_t deals, uint64_t seed, void* d_work,
                        int64_t work_bytes, const bb_plan2_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_plan2_values_pos",
                       R::plan2_values_pos(pos, n, d_w, w_stride, depth, candidates, deals, d_work, work_bytes, out)))
    return rc;
  plan2_values_host(pos->board, pos->hand, pos->combo, d_stream, n, d_w, w_stride, depth, candidates, deals, seed,
                    d_work, *out);
  return BB_OK;
}

int bb_plan2_values(bb_env* env, const uint64_t* d_stream, const bb_eval_weights* d_w, int64_t w_stride, int32_t depth,
                    int32_t candidates, int32_t deals, uint64_t seed, void* d_work, int64_t work_bytes,
                    const bb_plan2_out* out, void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_plan2_values",
                       R::plan2_values(env->n, d_w, w_stride, depth, candidates, deals, d_work, work_bytes, out)))
    return rc;
  plan2_values_host(env->board.data(), env->hand.data(), env->combo.data(), d_stream, env->n, d_w, w_stride, depth,
                    candidates, deals, seed, d_work, *out);
  return BB_OK;
}

int bb_playout_values_pos(const uint64_t* d_board, const int32_t* d_combo, const uint64_t* d_stream, int32_t n,
                          const bb_eval_weights* d_w, int64_t w_stride, int32_t depth, int32_t playouts, int32_t hands,
                          uint64_t seed, const bb_playout_out* out, void* stream) {
  (void)stream;
  if (int rc = refused(nullptr, "bb_playout_values_pos",
                       R::playout_values_pos(d_board, n, d_w, w_stride, depth, playouts, hands, out)))
    return rc;
  playout_values_host(d_board, d_combo, d_stream, n, d_w, w_stride, depth, playouts, hands, seed, *out);
  return BB_OK;
}

int bb_playout_values(bb_env* env, const uint64_t* d_stream, const bb_eval_weights* d_w, int64_t w_stride,
                      int32_t depth, int32_t playouts, int32_t hands, uint64_t seed, const bb_playout_out* out,
                      void* stream) {
  (void)stream;
  if (!env) return BB_ERR_ARG;
  if (int rc = refused(env, "bb_playout_values", R::playout_values(d_w, w_stride, depth, playouts, hands, out)))
    return rc;
  playout_values_host(env->board.data(), env->combo.data(), d_stream, env->n, d_w, w_stride, depth, playouts, hands,
                      seed, *out);
  return BB_OK;
}

}  // extern "C"
