// Sanitizer driver for the host backend's refill census (bb_refill_census_pos / bb_refill_census of
// csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by tests/test_refill_census_sanitize.py with
// -fsanitize=address,undefined.  Five boards with known counts (empty, full, the two checkerboards, a full board with
// one hole) and crowded random boards go into heap buffers of exactly n and n * 37 * 37 elements, with each output
// alone NULL and with both, stateless and through the handle.  The counts are held to the table below, the words to
// their own symmetry and popcount.  Any sanitizer report aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bbvec.h"

static int g_fail = 0;

static void expect(bool cond, const char* what, int i) {
  if (!cond) {
    fprintf(stderr, "MISMATCH %s at board %d\n", what, i);
    g_fail = 1;
  }
}

static void ok(int rc, const char* what, bb_env* env) {
  if (rc != BB_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, bb_last_error(env));
    exit(2);
  }
}

static const int NP = BB_NUM_PIECES, NW = BB_NUM_PIECES * BB_NUM_PIECES;

// count alone, words alone and both on `board`, into exactly sized buffers; returns the counts
static std::vector<int32_t> census(const std::vector<uint64_t>& board, const char* name) {
  const int n = (int)board.size();
  std::vector<int32_t> c1(n, -7), c2(n, -7);
  std::vector<uint64_t> w1((size_t)n * NW, 0xA5u), w2((size_t)n * NW, 0xA5u);
  const bb_census_out only_count{c1.data(), nullptr}, only_words{nullptr, w1.data()}, both{c2.data(), w2.data()};
  ok(bb_refill_census_pos(board.data(), n, &only_count, nullptr), "count alone", nullptr);
  ok(bb_refill_census_pos(board.data(), n, &only_words, nullptr), "words alone", nullptr);
  ok(bb_refill_census_pos(board.data(), n, &both, nullptr), "both", nullptr);
  expect(c1 == c2, name, -1);
  expect(w1 == w2, name, -2);
  for (int i = 0; i < n; ++i) {
    const uint64_t* w = &w1[(size_t)i * NW];
    int pop = 0;
    for (int a = 0; a < NP; ++a)
      for (int b = 0; b < NP; ++b) {
        const uint64_t x = w[a * NP + b];
        pop += __builtin_popcountll(x);
        expect((x >> NP) == 0, "high bits", i);
        expect(x == w[b * NP + a], "symmetric in (a, b)", i);
        for (int c = 0; c < NP; ++c) expect(((x >> c) & 1) == ((w[a * NP + c] >> b) & 1), "symmetric in (b, c)", i);
      }
    expect(pop == c1[i], "count is the popcount sum", i);
  }
  return c1;
}

int main(void) {
  // the table: counts of engine.py:174-224 over all 37^3 hands, from the project's C oracle
  const std::vector<uint64_t> known = {0ull, ~0ull, 0x55aa55aa55aa55aaull, 0x00aa55aa55aa55aaull,
                                       0xfffffffff7ffffffull};
  const int32_t want[5] = {BB_NUM_HANDS, 0, 125, 2995, 3997};
  const std::vector<int32_t> got = census(known, "known boards");
  for (int i = 0; i < 5; ++i) expect(got[i] == want[i], "known count", i);

  // crowded boards (fill 0.35 .. 0.9, no full line), splitmix64
  const int n2 = 48;
  const double fills[6] = {0.35, 0.5, 0.6, 0.7, 0.8, 0.9};
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&s]() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  std::vector<uint64_t> b2(n2);
  for (int i = 0; i < n2; ++i) {
    uint64_t B = 0;
    for (int c = 0; c < 64; ++c)
      if ((double)(next() >> 11) * (1.0 / 9007199254740992.0) < fills[i % 6]) B |= 1ull << c;
    for (int r = 0; r < 8; ++r)
      if (((B >> (8 * r)) & 0xFFull) == 0xFFull) B &= ~(1ull << (8 * r + (int)(next() % 8)));
    for (int c = 0; c < 8; ++c)
      if (((B >> c) & 0x0101010101010101ull) == 0x0101010101010101ull) B &= ~(1ull << (8 * (int)(next() % 8) + c));
    b2[i] = B;
  }
  const std::vector<int32_t> c2 = census(b2, "crowded boards");
  int partial = 0;
  for (int i = 0; i < n2; ++i) partial += c2[i] > 0 && c2[i] < BB_NUM_HANDS;
  expect(partial >= 8, "crowded boards with some and not all hands", -1);

  // the handle form on fresh games: every board empty, every hand fits
  const bb_reward_cfg cfg = {1.0, 0.01, -1.0, -0.05, 0.02, 0.5, 0.001};
  const int ne = 3;
  bb_env* env = nullptr;
  ok(bb_create(ne, 0, &cfg, 0, &env), "bb_create", nullptr);
  ok(bb_reset(env, nullptr, nullptr), "bb_reset", env);
  std::vector<int32_t> hc(ne, -7);
  std::vector<uint64_t> hw((size_t)ne * NW, 0xA5u);
  const bb_census_out hc_only{hc.data(), nullptr}, hw_only{nullptr, hw.data()};
  ok(bb_refill_census(env, &hc_only, nullptr), "bb_refill_census count", env);
  ok(bb_refill_census(env, &hw_only, nullptr), "bb_refill_census words", env);
  for (int i = 0; i < ne; ++i) expect(hc[i] == BB_NUM_HANDS, "handle count", i);
  for (size_t k = 0; k < hw.size(); ++k) expect(hw[k] == (1ull << NP) - 1, "handle words", (int)(k / NW));

  // argument errors are reported, not crashes; n == 0 does nothing
  int32_t one = 7;
  const bb_census_out o1{&one, nullptr}, none{nullptr, nullptr};
  if (bb_refill_census_pos(nullptr, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_census_pos(known.data(), -1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_census_pos(known.data(), 1, nullptr, nullptr) != BB_ERR_ARG ||
      bb_refill_census_pos(known.data(), 1, &none, nullptr) != BB_ERR_ARG ||
      bb_refill_census_pos(known.data(), 0, &o1, nullptr) != BB_OK || one != 7 ||
      bb_refill_census(nullptr, &o1, nullptr) != BB_ERR_ARG || bb_refill_census(env, &none, nullptr) != BB_ERR_ARG ||
      bb_refill_census(env, nullptr, nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks\n");
    g_fail = 1;
  }
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_refill_census under sanitizers: 5 known + %d crowded boards (%d partial), counts equal the table\n", n2,
         partial);
  return 0;
}
