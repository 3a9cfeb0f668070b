// Sanitizer driver for the host backend's per-action full-hand values (bb_plan_values_pos / bb_plan_values of
// csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by tests/test_plan_values_sanitize.py with
// -fsanitize=address,undefined.  It searches a handful of positions at depth 3 -- a fresh board with a whole hand
// (the largest tree), positions a few random moves into a game, the crafted "dead" position of
// tests/_afterstates_ref.py (legal moves, none of them safe) and a finished game -- into exactly sized buffers,
// with all outputs, each output alone and through the handle, and holds the results to bb_plan_actions_pos.
// Any sanitizer report aborts the process; a mismatch exits 1.
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
  const bb_greedy_weights w = {-7, 3, -1, 1, 5, -2, 50, 11};
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
  std::vector<int64_t> q((size_t)n * 192), q1((size_t)n * 192);
  std::vector<int32_t> rest((size_t)n * 192), leaves((size_t)n * 192), rest1((size_t)n * 192), leaves1((size_t)n * 192);
  std::vector<uint64_t> safe(3 * (size_t)n), safe1(3 * (size_t)n), safe2(3 * (size_t)n);
  const bb_plan_values_out all{q.data(), rest.data(), leaves.data(), safe.data()};
  ok(bb_plan_values_pos(&pos, n, &w, 3, &all, nullptr), "bb_plan_values_pos", nullptr);

  // each output alone, and the safe set at depth 2
  const bb_plan_values_out only_q{q1.data(), nullptr, nullptr, nullptr}, only_rest{nullptr, rest1.data(), nullptr, nullptr},
      only_leaves{nullptr, nullptr, leaves1.data(), nullptr}, only_safe{nullptr, nullptr, nullptr, safe1.data()},
      safe_d2{nullptr, nullptr, nullptr, safe2.data()};
  ok(bb_plan_values_pos(&pos, n, &w, 3, &only_q, nullptr), "q alone", nullptr);
  ok(bb_plan_values_pos(&pos, n, &w, 3, &only_rest, nullptr), "rest alone", nullptr);
  ok(bb_plan_values_pos(&pos, n, &w, 3, &only_leaves, nullptr), "leaves alone", nullptr);
  ok(bb_plan_values_pos(&pos, n, &w, 3, &only_safe, nullptr), "safe alone", nullptr);
  ok(bb_plan_values_pos(&pos, n, &w, 2, &safe_d2, nullptr), "safe at depth 2", nullptr);
  expect(q1 == q, "q alone", -1);
  expect(rest1 == rest, "rest alone", -1);
  expect(leaves1 == leaves, "leaves alone", -1);
  expect(safe1 == safe, "safe alone", -1);
  expect(safe2 == safe, "safe at depth 2", -1);

  // against bb_plan_actions_pos: value = max q, action = the lowest a attaining it, plan[1:] = rest, leaves = sum
  std::vector<int32_t> pa(n), pp(3 * (size_t)n), pl(n);
  std::vector<int64_t> pv(n);
  const bb_plan_out po{pa.data(), pv.data(), pp.data(), pl.data()};
  ok(bb_plan_actions_pos(&pos, n, &w, 3, &po, nullptr), "bb_plan_actions_pos", nullptr);
  for (int i = 0; i < n; ++i) {
    int64_t best = INT64_MIN, total = 0;
    int first = 0, nsafe = 0, nlegal = 0;
    for (int a = 0; a < 192; ++a) {
      const size_t o = (size_t)i * 192 + (size_t)a;
      const bool legal = leaves[o] > 0, is_safe = (safe[3 * (size_t)i + (a >> 6)] >> (a & 63)) & 1ull;
      expect(legal == (q[o] != INT64_MIN) && legal == (rest[o] != -1) && (!is_safe || legal), "illegal entries", i);
      if (q[o] > best) best = q[o], first = a;
      total += leaves[o];
      nsafe += is_safe;
      nlegal += legal;
    }
    expect(best == pv[i] && total == pl[i], "value / leaves against bb_plan_actions", i);
    if (total) {
      const int32_t r = rest[(size_t)i * 192 + (size_t)first];
      const int a2 = r & 0xFF, a3 = (r >> 8) & 0xFF;
      expect(first == pa[i] && (a2 == 0xFF ? -1 : a2) == pp[3 * (size_t)i + 1] &&
                 (a3 == 0xFF ? -1 : a3) == pp[3 * (size_t)i + 2],
             "action / plan against bb_plan_actions", i);
    }
    if (i == 0) expect(total > 50000 && nsafe == nlegal, "fresh board: every move is safe", i);
    if (i == kDead) expect(nlegal == 16 && nsafe == 0, "dead: 16 legal moves, none safe", i);
    if (i == kOver) expect(nlegal == 0, "game over: nothing legal", i);
    if (i == kLast) expect(nlegal == 16 && nsafe == 16 && total == 16, "last piece: every move is a refill", i);
  }

  // the handle form on the played positions
  std::vector<int64_t> qh((size_t)played * 192);
  std::vector<uint64_t> sh(3 * (size_t)played);
  const bb_plan_values_out oh{qh.data(), nullptr, nullptr, sh.data()};
  ok(bb_plan_values(env, &w, 3, &oh, nullptr), "bb_plan_values", env);
  for (size_t k = 0; k < qh.size(); ++k) expect(qh[k] == q[k], "handle q", (int)(k / 192));
  for (size_t k = 0; k < sh.size(); ++k) expect(sh[k] == safe[k], "handle safe", (int)(k / 3));

  // argument errors are reported, not crashes
  const bb_plan_values_out none{nullptr, nullptr, nullptr, nullptr};
  if (bb_plan_values_pos(&pos, n, &w, 3, &none, nullptr) != BB_ERR_ARG || bb_plan_values_pos(&pos, n, &w, 4, &all, nullptr) != BB_ERR_ARG ||
      bb_plan_values_pos(&pos, -1, &w, 3, &all, nullptr) != BB_ERR_ARG || bb_plan_values_pos(&pos, 0, &w, 3, &all, nullptr) != BB_OK ||
      bb_plan_values(env, nullptr, 3, &all, nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks\n");
    g_fail = 1;
  }
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_plan_values under sanitizers: %d positions at depth 3, consistent with bb_plan_actions\n", n);
  return 0;
}
