// Sanitizer driver for the host backend's per-position weights (bb_greedy_actions_each(_pos) and
// bb_plan_actions_each(_pos) of csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by
// tests/test_weights_each_sanitize.py with -fsanitize=address,undefined.  It searches a fresh board with a whole
// hand, positions a few random moves into a game, the crafted "dead" position of tests/_afterstates_ref.py, a
// finished game and a last-piece position at depth 3, every position under a row of its own, with the rows in a
// heap buffer of exactly n rows (an off-by-one row read is the error this is for), and holds every result to the
// uniform call made with that row.  Any sanitizer report aborts the process; a mismatch exits 1.
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

  // one row per position, all different, the last one at the ends of int32; exactly n rows on the heap
  bb_greedy_weights* rows = (bb_greedy_weights*)malloc(sizeof(bb_greedy_weights) * (size_t)n);
  if (!rows) return 2;
  for (int i = 0; i < n; ++i)
    rows[i] = bb_greedy_weights{100 - 37 * i, 3 * i - 5, -30 + 11 * i, i - 2, 5 - i, 1 + i, -100000 + 25000 * i, 7 * i};
  rows[n - 1] = bb_greedy_weights{INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX};

  // the per-position calls into exactly sized outputs
  std::vector<int32_t> ea(n), ep(3 * (size_t)n), el(n), ga(n);
  std::vector<int64_t> ev(n), gv(n);
  const bb_plan_out eo{ea.data(), ev.data(), ep.data(), el.data()};
  ok(bb_plan_actions_each_pos(&pos, n, rows, 3, &eo, nullptr), "bb_plan_actions_each_pos", nullptr);
  ok(bb_greedy_actions_each_pos(&pos, n, rows, ga.data(), gv.data(), nullptr), "bb_greedy_actions_each_pos", nullptr);

  // against the uniform calls, one position and one row at a time
  int differ = 0;
  for (int i = 0; i < n; ++i) {
    const bb_positions one{board.data() + i, hand.data() + i, combo.data() + i, nullptr};
    int32_t a = -7, p[3] = {-7, -7, -7}, l = -7, a1 = -7;
    int64_t v = 5, v1 = 5;
    const bb_plan_out uo{&a, &v, p, &l};
    ok(bb_plan_actions_pos(&one, 1, &rows[i], 3, &uo, nullptr), "bb_plan_actions_pos", nullptr);
    expect(ea[i] == a && ev[i] == v && el[i] == l, "plan action / value / leaves", i);
    expect(ep[3 * (size_t)i] == p[0] && ep[3 * (size_t)i + 1] == p[1] && ep[3 * (size_t)i + 2] == p[2], "plan", i);
    ok(bb_greedy_actions_pos(&one, 1, &rows[i], &a1, &v1, nullptr), "bb_greedy_actions_pos", nullptr);
    expect(ga[i] == a1 && gv[i] == v1, "greedy action / value", i);
    // the neighbouring row would have given another answer somewhere: the check above can tell an off-by-one
    if (i + 1 < n) {
      int64_t vn = 5;
      const bb_plan_out no{&a, &vn, nullptr, nullptr};
      ok(bb_plan_actions_pos(&one, 1, &rows[i + 1], 3, &no, nullptr), "bb_plan_actions_pos (next row)", nullptr);
      differ += vn != v;
    }
    if (i == 0) expect(l > 50000, "fresh board: the largest tree", i);
    if (i == kDead) expect(l == 16, "dead: 16 sequences of one move", i);
    if (i == kOver) expect(a == 0 && v == INT64_MIN && l == 0 && p[0] == -1, "game over: nothing legal", i);
    if (i == kLast) expect(l == 16 && p[1] == -1, "last piece: every move is a refill", i);
  }
  expect(differ >= played, "neighbouring rows give other values", -1);

  // NULL optional outputs
  std::vector<int32_t> ea2(n), ga2(n);
  const bb_plan_out only_action{ea2.data(), nullptr, nullptr, nullptr};
  ok(bb_plan_actions_each_pos(&pos, n, rows, 3, &only_action, nullptr), "action alone", nullptr);
  ok(bb_greedy_actions_each_pos(&pos, n, rows, ga2.data(), nullptr, nullptr), "greedy action alone", nullptr);
  expect(ea2 == ea && ga2 == ga, "action alone", -1);

  // the handle forms on the played positions: num_envs rows, again exactly sized
  bb_greedy_weights* hrows = (bb_greedy_weights*)malloc(sizeof(bb_greedy_weights) * (size_t)played);
  if (!hrows) return 2;
  for (int i = 0; i < played; ++i) hrows[i] = rows[i];
  std::vector<int32_t> ha(played), hp(3 * (size_t)played), hl(played), hga(played);
  std::vector<int64_t> hv(played), hgv(played);
  const bb_plan_out ho{ha.data(), hv.data(), hp.data(), hl.data()};
  ok(bb_plan_actions_each(env, hrows, 3, &ho, nullptr), "bb_plan_actions_each", env);
  ok(bb_greedy_actions_each(env, hrows, hga.data(), hgv.data(), nullptr), "bb_greedy_actions_each", env);
  for (int i = 0; i < played; ++i) {
    expect(ha[i] == ea[i] && hv[i] == ev[i] && hl[i] == el[i] && hp[3 * (size_t)i + 2] == ep[3 * (size_t)i + 2],
           "handle plan", i);
    expect(hga[i] == ga[i] && hgv[i] == gv[i], "handle greedy", i);
  }

  // argument errors are reported, not crashes
  if (bb_plan_actions_each_pos(&pos, n, nullptr, 3, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_each_pos(&pos, 0, rows, 3, &eo, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_each_pos(&pos, n, rows, 4, &eo, nullptr) != BB_ERR_ARG ||
      bb_greedy_actions_each_pos(&pos, n, nullptr, ga.data(), nullptr, nullptr) != BB_ERR_ARG ||
      bb_plan_actions_each(env, nullptr, 3, &ho, nullptr) != BB_ERR_ARG ||
      bb_greedy_actions_each(env, hrows, nullptr, nullptr, nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks\n");
    g_fail = 1;
  }
  free(hrows);
  free(rows);
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_*_actions_each under sanitizers: %d positions at depth 3, consistent with the uniform calls\n", n);
  return 0;
}
