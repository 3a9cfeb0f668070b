// Sanitizer driver for the host backend's hand-safe mask call (bb_safe_mask_pos / bb_safe_mask of
// csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by tests/test_safe_mask_sanitize.py with
// -fsanitize=address,undefined.  Two position sets -- games a few random moves in plus crafted positions (the
// "dead" one with legal moves and none safe, a finished game, a last piece), and crowded random boards under
// random hands with every used pattern -- go through both modes into exactly sized buffers, stateless and through
// the handle, and are held to bb_plan_values_pos' safe words at depth 2 and its legal set (q != INT64_MIN).
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

// both modes on (board, hand) against bb_plan_values_pos at depth 2; returns the number of fallback positions
static int check_set(const std::vector<uint64_t>& board, const std::vector<uint32_t>& hand, const char* name) {
  const int n = (int)board.size();
  const bb_greedy_weights w = {0, 0, 0, 0, 0, 0, 0, 0};
  const bb_positions pos{board.data(), hand.data(), nullptr, nullptr};
  std::vector<int64_t> q((size_t)n * 192);
  std::vector<uint64_t> safe(3 * (size_t)n), m0(3 * (size_t)n), m1(3 * (size_t)n);
  const bb_plan_values_out pv{q.data(), nullptr, nullptr, safe.data()};
  ok(bb_plan_values_pos(&pos, n, &w, 2, &pv, nullptr), "bb_plan_values_pos", nullptr);
  ok(bb_safe_mask_pos(&pos, n, BB_SAFE_WORDS, m0.data(), nullptr), "bb_safe_mask_pos mode 0", nullptr);
  ok(bb_safe_mask_pos(&pos, n, BB_SAFE_OR_LEGAL, m1.data(), nullptr), "bb_safe_mask_pos mode 1", nullptr);
  int fallback = 0;
  for (int i = 0; i < n; ++i) {
    uint64_t legal[3] = {0, 0, 0};
    for (int a = 0; a < 192; ++a)
      if (q[(size_t)i * 192 + (size_t)a] != INT64_MIN) legal[a >> 6] |= 1ull << (a & 63);
    const uint64_t* s = &safe[3 * (size_t)i];
    const bool any = (s[0] | s[1] | s[2]) != 0;
    fallback += !any && (legal[0] | legal[1] | legal[2]) != 0;
    for (int p = 0; p < 3; ++p) {
      expect(m0[3 * (size_t)i + p] == s[p], name, i);
      expect(m1[3 * (size_t)i + p] == (any ? s[p] : legal[p]), name, i);
    }
  }
  return fallback;
}

int main(void) {
  const bb_reward_cfg cfg = {1.0, 0.01, -1.0, -0.05, 0.02, 0.5, 0.001};
  const int played = 12;

  // set 1: a game each, position i after 2*i random legal moves (0: the fresh board), then crafted positions
  bb_env* env = nullptr;
  std::vector<uint64_t> seeds(played), raw(4 * (size_t)played);
  std::vector<uint8_t> has(played, 1);
  for (int i = 0; i < played; ++i) {
    seeds[i] = 300 + (uint64_t)i;
    ok(bb_pcg64_seed(seeds[i], &raw[4 * (size_t)i]), "bb_pcg64_seed", nullptr);
  }
  ok(bb_create(played, 0, &cfg, 0, &env), "bb_create", nullptr);
  ok(bb_seed(env, seeds.data(), has.data(), raw.data()), "bb_seed", env);
  ok(bb_reset(env, nullptr, nullptr), "bb_reset", env);
  std::vector<uint64_t> board(played), mb(3 * (size_t)played);
  std::vector<uint32_t> hand(played);
  std::vector<int32_t> act(played);
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
  bb_state_view sv{board.data(), hand.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr};
  ok(bb_get_state(env, &sv), "bb_get_state", env);
  expect(board[0] == 0, "fresh board", 0);

  // the handle form on the played positions, both modes, into exactly sized buffers
  std::vector<uint64_t> p0(3 * (size_t)played), p1(3 * (size_t)played), h0(3 * (size_t)played), h1(3 * (size_t)played);
  const bb_positions ppos{board.data(), hand.data(), nullptr, nullptr};
  ok(bb_safe_mask_pos(&ppos, played, 0, p0.data(), nullptr), "played mode 0", nullptr);
  ok(bb_safe_mask_pos(&ppos, played, 1, p1.data(), nullptr), "played mode 1", nullptr);
  ok(bb_safe_mask(env, 0, h0.data(), nullptr), "bb_safe_mask mode 0", env);
  ok(bb_safe_mask(env, 1, h1.data(), nullptr), "bb_safe_mask mode 1", env);
  expect(h0 == p0, "handle mode 0", -1);
  expect(h1 == p1, "handle mode 1", -1);

  // crafted: two free cells per row and column, never adjacent; SINGLE, DOMINO_H, (used) SQUARE_3x3
  uint64_t tight = ~0ull;
  for (int i = 0; i < 8; ++i) tight &= ~((1ull << (i * 8 + i)) | (1ull << (i * 8 + (i + 4) % 8)));
  board.push_back(tight);  // dead: 16 legal moves, none safe -> mode 1 falls back
  hand.push_back(0u | (1u << 6) | (36u << 12) | (1u << 20));
  board.push_back(tight);  // game over
  hand.push_back(17u | (1u << 6) | (36u << 12) | (1u << 21));
  board.push_back(tight);  // one piece left: every move is a refill
  hand.push_back(0u | (1u << 6) | (36u << 12) | (1u << 19) | (1u << 20));
  board.push_back(0);      // a piece id outside the table in an unused slot places nowhere
  hand.push_back(0u | (1u << 6) | (63u << 12));
  const int fb1 = check_set(board, hand, "set 1");
  expect(fb1 >= 1, "set 1 has a fallback position", -1);

  // set 2: crowded boards (fill 0.35 .. 0.9, no full line) under random hands, every used pattern
  const int n2 = 420;
  const double fills[6] = {0.35, 0.5, 0.6, 0.7, 0.8, 0.9};
  const uint32_t used[7] = {0, 1, 2, 4, 3, 5, 6};
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&s]() {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  std::vector<uint64_t> b2(n2);
  std::vector<uint32_t> h2(n2);
  for (int i = 0; i < n2; ++i) {
    uint64_t B = 0;
    for (int c = 0; c < 64; ++c)
      if ((double)(next() >> 11) * (1.0 / 9007199254740992.0) < fills[i % 6]) B |= 1ull << c;
    for (int r = 0; r < 8; ++r)
      if (((B >> (8 * r)) & 0xFFull) == 0xFFull) B &= ~(1ull << (8 * r + (int)(next() % 8)));
    for (int c = 0; c < 8; ++c)
      if (((B >> c) & 0x0101010101010101ull) == 0x0101010101010101ull) B &= ~(1ull << (8 * (int)(next() % 8) + c));
    b2[i] = B;
    h2[i] = (uint32_t)(next() % BB_NUM_PIECES) | ((uint32_t)(next() % BB_NUM_PIECES) << 6) |
            ((uint32_t)(next() % BB_NUM_PIECES) << 12) | (used[(i / 6) % 7] << 18);
  }
  const int fb2 = check_set(b2, h2, "set 2");
  expect(fb2 >= 5, "set 2 has fallback positions", -1);

  // argument errors are reported, not crashes; n == 0 does nothing
  std::vector<uint64_t> one(3, 7);
  if (bb_safe_mask_pos(nullptr, 1, 0, one.data(), nullptr) != BB_ERR_ARG ||
      bb_safe_mask_pos(&ppos, -1, 0, one.data(), nullptr) != BB_ERR_ARG ||
      bb_safe_mask_pos(&ppos, 1, 2, one.data(), nullptr) != BB_ERR_ARG ||
      bb_safe_mask_pos(&ppos, 1, 0, nullptr, nullptr) != BB_ERR_ARG ||
      bb_safe_mask_pos(&ppos, 0, 1, one.data(), nullptr) != BB_OK || one[0] != 7 ||
      bb_safe_mask(nullptr, 0, one.data(), nullptr) != BB_ERR_ARG ||
      bb_safe_mask(env, 3, one.data(), nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks\n");
    g_fail = 1;
  }
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_safe_mask under sanitizers: %d + %d positions, both modes equal bb_plan_values (%d + %d fallbacks)\n",
         (int)board.size(), n2, fb1, fb2);
  return 0;
}
