// Sanitizer driver for the host backend's shape terms and the search with them (bb_board_terms(_pos) and
// bb_plan_actions_ext(_pos) of csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by tests/test_eval_terms_sanitize.py
// with -fsanitize=address,undefined.  Positions a few random moves into a game, the crafted "dead" position of
// tests/_afterstates_ref.py, a finished game and a last-piece position, searched at depth 3 with one row of twelve
// weights per position in a heap buffer of exactly n rows (an off-by-one row read is the error this is for: the
// neighbouring row is checked to give another value), with one shared row in a buffer of exactly one row, and
// through the handle; the terms into an output of exactly 4 n words.  Rows whose shape weights are 0 are held to
// bb_plan_actions_pos.  Any sanitizer report aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bbvec.h"

static int g_fail = 0;

static void expect(bool cond, const char* what, int i) {
  if (!cond) {
    fprintf(stderr, "MISMATCH %s at position %d\n", what, i);
    g_fail = 1;
  }
}

static void ok(int rc, const char* what, bb_env* env) {
  if (rc != BB_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, bb_last_error(env));
    exit(2);
  }
}

int main(void) {
  const bb_reward_cfg cfg = {1.0, 0.01, -1.0, -0.05, 0.02, 0.5, 0.001};
  const int played = 6;
  const int n = played + 3;

  // positions 0 .. played-1: a game each, position i after 2*i random legal moves (0: the fresh board)
  bb_env* env = nullptr;
  std::vector<uint64_t> seeds(played), raw(4 * (size_t)played);
  std::vector<uint8_t> has(played, 1);
  for (int i = 0; i < played; ++i) {
    seeds[i] = 100 + (uint64_t)i;
    ok(bb_pcg64_seed(seeds[i], &raw[4 * (size_t)i]), "bb_pcg64_seed", nullptr);
  }
  ok(bb_create(played, 0, &cfg, 0, &env), "bb_create", nullptr);
  ok(bb_seed(env, seeds.data(), has.data(), raw.data()), "bb_seed", env);
  ok(bb_reset(env, nullptr, nullptr), "bb_reset", env);
  std::vector<uint64_t> board(n), mb(3 * (size_t)played);
  std::vector<uint32_t> hand(n);
  std::vector<int32_t> combo(n, 0), act(played);
  std::vector<float> rw(played);
  std::vector<uint8_t> tm(played);
  for (int s = 0; s < 2 * (played - 1); ++s) {
    ok(bb_obs(env, nullptr, nullptr, nullptr, mb.data(), nullptr), "bb_obs", env);
    ok(bb_random_actions(mb.data(), played, 0xB10C, (uint64_t)s, 0, act.data(), nullptr), "bb_random_actions", env);
    for (int i = 0; i < played; ++i)
      if (s >= 2 * i) act[i] = -1;  // env i stops after 2*i moves: an invalid action changes nothing
    bb_step_out so{rw.data(), tm.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr};
    ok(bb_step(env, act.data(), &so, nullptr), "bb_step", env);
  }
  bb_state_view sv{board.data(), hand.data(), nullptr, combo.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr};
  ok(bb_get_state(env, &sv), "bb_get_state", env);
  expect(board[0] == 0, "fresh board", 0);

  // crafted: two free cells per row and column, never adjacent; SINGLE, DOMINO_H, (used) SQUARE_3x3
  uint64_t tight = ~0ull;
  for (int i = 0; i < 8; ++i) tight &= ~((1ull << (i * 8 + i)) | (1ull << (i * 8 + (i + 4) % 8)));
  const int kDead = played, kOver = played + 1, kLast = played + 2;
  board[kDead] = tight;
  hand[kDead] = 0u | (1u << 6) | (36u << 12) | (1u << 20);
  board[kOver] = tight;
  hand[kOver] = 17u | (1u << 6) | (36u << 12) | (1u << 21);
  board[kLast] = tight;  // one piece left: every first move is a refill
  hand[kLast] = 0u | (1u << 6) | (36u << 12) | (1u << 19) | (1u << 20);
  combo[kLast] = 9;
  const bb_positions pos{board.data(), hand.data(), combo.data(), nullptr};

  // ---- the terms: exactly 4 n words on the heap, known boards
  {
    const int m = 4;
    uint64_t* b = (uint64_t*)malloc(sizeof(uint64_t) * m);
    int32_t* t = (int32_t*)malloc(sizeof(int32_t) * 4 * m);
    if (!b || !t) return 2;
    b[0] = 0ull, b[1] = ~0ull, b[2] = 0x55AA55AA55AA55AAull, b[3] = tight;
    ok(bb_board_terms_pos(b, m, t, nullptr), "bb_board_terms_pos", nullptr);
    expect(t[0] == 32 && t[1] == 36 && t[2] == 64 && t[3] == 37, "terms of the empty board", 0);
    expect(t[4] == 0 && t[5] == 0 && t[6] == 0 && t[7] == 0, "terms of the full board", 1);
    expect(t[8] == 128 && t[9] == 0 && t[10] == 0 && t[11] == 5, "terms of the checker board", 2);
    expect(t[12] == 64 && t[13] == 0 && t[14] == 0 && t[15] == 3, "terms of the tight board", 3);  // 16 holes
    ok(bb_board_terms_pos(b, 0, t, nullptr), "bb_board_terms_pos n = 0", nullptr);
    int32_t* ht = (int32_t*)malloc(sizeof(int32_t) * 4 * played);
    int32_t* pt = (int32_t*)malloc(sizeof(int32_t) * 4 * played);
    if (!ht || !pt) return 2;
    ok(bb_board_terms(env, ht, nullptr), "bb_board_terms", env);
    ok(bb_board_terms_pos(board.data(), played, pt, nullptr), "bb_board_terms_pos (played)", nullptr);
    for (int i = 0; i < 4 * played; ++i) expect(ht[i] == pt[i], "handle terms", i / 4);
    if (bb_board_terms_pos(nullptr, m, t, nullptr) != BB_ERR_ARG || bb_board_terms_pos(b, -1, t, nullptr) != BB_ERR_ARG ||
        bb_board_terms_pos(b, m, nullptr, nullptr) != BB_ERR_ARG || bb_board_terms(env, nullptr, nullptr) != BB_ERR_ARG) {
      fprintf(stderr, "argument checks (terms)\n");
      g_fail = 1;
    }
    free(pt);
    free(ht);
    free(t);
    free(b);
  }

  // ---- the search: one row per position, all different, the last one at the ends of int32; exactly n rows
  bb_eval_weights* rows = (bb_eval_weights*)malloc(sizeof(bb_eval_weights) * (size_t)n);
  if (!rows) return 2;
  for (int i = 0; i < n; ++i)
    rows[i] = bb_eval_weights{{100 - 37 * i, 3 * i - 5, -30 + 11 * i, i - 2, 5 - i, 1 + i, -100000 + 25000 * i, 7 * i},
                              -3 + 2 * i, 4 - i, 2 + 3 * i, 25 - 9 * i};
  rows[n - 1] = bb_eval_weights{{INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX},
                                INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX};
  std::vector<int32_t> ea(n), ep(3 * (size_t)n), el(n);
  std::vector<int64_t> ev(n);
  const bb_plan_out eo{ea.data(), ev.data(), ep.data(), el.data()};
  ok(bb_plan_actions_ext_pos(&pos, n, rows, 1, 3, &eo, nullptr), "bb_plan_actions_ext_pos", nullptr);

  int differ = 0;
  for (int i = 0; i < n; ++i) {
    const bb_positions one{board.data() + i, hand.data() + i, combo.data() + i, nullptr};
    // the position alone under its row as the one shared row, in a buffer of exactly one row
    bb_eval_weights* shared = (bb_eval_weights*)malloc(sizeof(bb_eval_weights));
    if (!shared) return 2;
    *shared = rows[i];
    int32_t a = -7, p[3] = {-7, -7, -7}, l = -7;
    int64_t v = 5;
    const bb_plan_out uo{&a, &v, p, &l};
    ok(bb_plan_actions_ext_pos(&one, 1, shared, 0, 3, &uo, nullptr), "bb_plan_actions_ext_pos (shared row)", nullptr);
    expect(ea[i] == a && ev[i] == v && el[i] == l, "ext action / value / leaves", i);
    expect(ep[3 * (size_t)i] == p[0] && ep[3 * (size_t)i + 1] == p[1] && ep[3 * (size_t)i + 2] == p[2], "ext plan", i);
    // the neighbouring row would have given another value: the check above can tell an off-by-one
    if (i + 1 < n) {
      int64_t vn = 5;
      int32_t an = -7;
      *shared = rows[i + 1];
      const bb_plan_out no{&an, &vn, nullptr, nullptr};
      ok(bb_plan_actions_ext_pos(&one, 1, shared, 0, 3, &no, nullptr), "bb_plan_actions_ext_pos (next row)", nullptr);
      differ += vn != v;
    }
    // the shape weights at 0: the eight-weight search, output for output
    *shared = rows[i];
    shared->perimeter = shared->room3 = shared->room5 = shared->fits = 0;
    int32_t a0 = -7, p0[3] = {-7, -7, -7}, l0 = -7, a1 = -7, p1[3] = {-7, -7, -7}, l1 = -7;
    int64_t v0 = 5, v1 = 5;
    const bb_plan_out zo{&a0, &v0, p0, &l0}, po{&a1, &v1, p1, &l1};
    ok(bb_plan_actions_ext_pos(&one, 1, shared, 0, 3, &zo, nullptr), "bb_plan_actions_ext_pos (zero shape)", nullptr);
    ok(bb_plan_actions_pos(&one, 1, &rows[i].base, 3, &po, nullptr), "bb_plan_actions_pos", nullptr);
    expect(a0 == a1 && v0 == v1 && l0 == l1 && p0[0] == p1[0] && p0[1] == p1[1] && p0[2] == p1[2], "zero shape weights", i);
    free(shared);
    if (i == 0) expect(l > 50000, "fresh board: the largest tree", i);
    if (i == kDead) expect(l == 16, "dead: 16 sequences of one move", i);
    if (i == kOver) expect(a == 0 && v == INT64_MIN && l == 0 && p[0] == -1, "game over: nothing legal", i);
    if (i == kLast) expect(l == 16 && p[1] == -1, "last piece: every move is a refill", i);
  }
  expect(differ >= played, "neighbouring rows give other values", -1);

  // NULL optional outputs, and n == 0
  std::vector<int32_t> ea2(n);
  const bb_plan_out only_action{ea2.data(), nullptr, nullptr, nullptr};
  ok(bb_plan_actions_ext_pos(&pos, n, rows, 1, 3, &only_action, nullptr), "action alone", nullptr);
  expect(ea2 == ea, "action alone", -1);
  ok(bb_plan_actions_ext_pos(&pos, 0, rows, 1, 3, &only_action, nullptr), "n = 0", nullptr);

  // the handle form on the played positions: num_envs rows, again exactly sized, then one shared row
  bb_eval_weights* hrows = (bb_eval_weights*)malloc(sizeof(bb_eval_weights) * (size_t)played);
  if (!hrows) return 2;
  for (int i = 0; i < played; ++i) hrows[i] = rows[i];
  std::vector<int32_t> ha(played), hp(3 * (size_t)played), hl(played);
  std::vector<int64_t> hv(played);
  const bb_plan_out ho{ha.data(), hv.data(), hp.data(), hl.data()};
  ok(bb_plan_actions_ext(env, hrows, 1, 3, &ho, nullptr), "bb_plan_actions_ext", env);
  for (int i = 0; i < played; ++i)
    expect(ha[i] == ea[i] && hv[i] == ev[i] && hl[i] == el[i] && hp[3 * (size_t)i + 2] == ep[3 * (size_t)i + 2],
           "handle ext", i);
  ok(bb_plan_actions_ext(env, hrows, 0, 3, &ho, nullptr), "bb_plan_actions_ext (shared row)", env);
  expect(ha[0] == ea[0] && hv[0] == ev[0], "handle ext, shared row", 0);

  // argument errors are reported, not crashes
  if (bb_plan_actions_ext_pos(&pos, n, nullptr, 1, 3, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext_pos(&pos, -1, rows, 1, 3, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext_pos(&pos, n, rows, 2, 3, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext_pos(&pos, n, rows, -1, 3, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext_pos(&pos, n, rows, 1, 4, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext_pos(&pos, n, rows, 1, 3, nullptr, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext(env, nullptr, 1, 3, &ho, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_ext(env, hrows, 12, 3, &ho, nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks (search)\n");
    g_fail = 1;
  }
  free(hrows);
  free(rows);
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_board_terms / bb_plan_actions_ext under sanitizers: %d positions at depth 3, consistent\n", n);
  return 0;
}
