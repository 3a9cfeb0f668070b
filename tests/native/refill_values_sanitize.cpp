// Sanitizer driver for the host backend's dealt next-hand values and plan play (bb_refill_values_pos /
// bb_refill_values / bb_play_plan_pos of csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by
// tests/test_refill_values_sanitize.py with -fsanitize=address,undefined.  The fixed case (seed 1, stream = i, 8 deals
// on five named boards, depth 2) goes into heap buffers of exactly n * deals elements with each output NULL in turn,
// stateless and through the handle, with and without the combo and stream columns; hands, attempts and values are
// held to the table below (tests/_refill_values_ref.py's answers).  Every dealt hand is then played with
// bb_play_plan_pos, each of its outputs NULL in turn.  Any sanitizer report aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bbvec.h"

static int g_fail = 0;

static void expect(bool cond, const char* what, int i) {
  if (!cond) {
    fprintf(stderr, "MISMATCH %s at %d\n", what, i);
    g_fail = 1;
  }
}

static void ok(int rc, const char* what, bb_env* env) {
  if (rc != BB_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, bb_last_error(env));
    exit(2);
  }
}

static const int N = 5, M = 8;
static const uint64_t kBoards[N] = {0ull, ~0ull, 0x55aa55aa55aa55aaull, 0x00aa55aa55aa55aaull, 0xfffffffff7ffffffull};
static const uint32_t kHands[N][M] = {
    {88160, 132630, 107293, 128917, 196, 116580, 147544, 123978},
    {148992, 95577, 61899, 41733, 24608, 46423, 37329, 135490},
    {1952, 71509, 90696, 12291, 144259, 16643, 22737, 24779},
    {74015, 118978, 9042, 119104, 118976, 136, 37071, 33027},
    {94213, 123904, 715, 124160, 2067, 2264, 352, 103424}};
static const int32_t kAttempts[N][M] = {{1, 1, 1, 1, 1, 1, 1, 1},
                                        {-100, -100, -100, -100, -100, -100, -100, -100},
                                        {-100, -100, -100, 48, -100, 25, -100, -100},
                                        {8, 22, 48, 34, 25, 1, 3, 5},
                                        {17, 25, 49, 40, 6, 1, 19, 2}};
static const int64_t kValues2[N][M] = {  // depth 2 under the default weights
    {20, 19, 25, 20, 52, 12, 17, 28},
    {-100000, -100000, -100000, -100000, -100000, -100000, -100000, -100000},
    {-100996, -100000, -100940, -884, -100968, -891, -100000, -100968},
    {-726, -722, -787, -782, -689, -660, -724, -616},
    {1635, 1629, 1640, 1632, 1630, 1628, 1636, 1628}};
static const bb_greedy_weights kW = {100, 0, -30, -2, 0, 1, -100000, 0};

static void check_table(const std::vector<uint32_t>* h, const std::vector<int64_t>* v, const std::vector<int32_t>* a,
                        const char* what) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < M; ++j) {
      if (h) expect((*h)[i * M + j] == kHands[i][j], what, i * M + j);
      if (v) expect((*v)[i * M + j] == kValues2[i][j], what, i * M + j);
      if (a) expect((*a)[i * M + j] == kAttempts[i][j], what, i * M + j);
    }
}

int main(void) {
  const std::vector<uint64_t> board(kBoards, kBoards + N);
  const std::vector<int32_t> zero_combo(N, 0);
  std::vector<uint64_t> ident(N);
  for (int i = 0; i < N; ++i) ident[i] = (uint64_t)i;

  // each output alone, every pair and all three, into exactly sized buffers; NULL columns and explicit ones
  for (int mask = 1; mask < 8; ++mask)
    for (int cols = 0; cols < 2; ++cols) {
      std::vector<uint32_t> h(N * M, 0xA5A5A5A5u);
      std::vector<int64_t> v(N * M, -7);
      std::vector<int32_t> a(N * M, -7);
      const bb_refill_values_out o{mask & 1 ? h.data() : nullptr, mask & 2 ? v.data() : nullptr,
                                   mask & 4 ? a.data() : nullptr};
      ok(bb_refill_values_pos(board.data(), cols ? zero_combo.data() : nullptr, cols ? ident.data() : nullptr, N, &kW,
                              2, M, 1, &o, nullptr),
         "bb_refill_values_pos", nullptr);
      check_table(mask & 1 ? &h : nullptr, mask & 2 ? &v : nullptr, mask & 4 ? &a : nullptr, "fixed case");
      if (!(mask & 1)) expect(h[0] == 0xA5A5A5A5u && h[N * M - 1] == 0xA5A5A5A5u, "hand untouched", mask);
      if (!(mask & 2)) expect(v[0] == -7 && v[N * M - 1] == -7, "value untouched", mask);
      if (!(mask & 4)) expect(a[0] == -7 && a[N * M - 1] == -7, "attempts untouched", mask);
    }

  // the bounds of deals and depth: one deal, 1,024 deals, depths 1 and 3 on a single board
  for (int deals : {1, BB_REFILL_MAX_DEALS}) {
    std::vector<int32_t> a(deals, -7);
    std::vector<int64_t> v(deals, -7);
    const bb_refill_values_out o{nullptr, v.data(), a.data()};
    ok(bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 1, deals, 1, &o, nullptr), "deals bound", nullptr);
    for (int j = 0; j < deals; ++j) expect(a[j] == 1 && v[j] != -7, "an empty board accepts the first draw", j);
    expect(a[0] == kAttempts[0][0], "deal 0 is deal 0 whatever the number of deals", deals);
  }
  {
    std::vector<uint32_t> h(N * M);
    std::vector<int64_t> v3(N * M);
    const bb_refill_values_out o{h.data(), v3.data(), nullptr};
    ok(bb_refill_values_pos(board.data(), nullptr, nullptr, N, &kW, 3, M, 1, &o, nullptr), "depth 3", nullptr);
    check_table(&h, nullptr, nullptr, "depth 3 hands");
    for (int j = 0; j < M; ++j) expect(v3[M + j] == kW.dead, "a full board: the dead weight at every depth", j);

    // every dealt hand played out greedily through bb_play_plan_pos: plan = the best plan of bb_plan_actions_pos
    const int n = N * M;
    std::vector<uint64_t> b(n);
    for (int k = 0; k < n; ++k) b[k] = kBoards[k / M];
    std::vector<int32_t> action(n), plan(3 * (size_t)n);
    const bb_positions pos{b.data(), h.data(), nullptr, nullptr};
    const bb_plan_out po{action.data(), nullptr, plan.data(), nullptr};
    ok(bb_plan_actions_pos(&pos, n, &kW, 3, &po, nullptr), "bb_plan_actions_pos", nullptr);
    std::vector<uint64_t> ob(n), ob2(n);
    std::vector<uint32_t> oh(n);
    std::vector<int32_t> oc(n), ol(n), os(n), os2(n);
    std::vector<int64_t> osc(n);
    const bb_play_plan_out all{ob.data(), oh.data(), oc.data(), ol.data(), osc.data(), os.data()};
    ok(bb_play_plan_pos(&pos, n, plan.data(), &all, nullptr), "bb_play_plan_pos", nullptr);
    for (int drop = 0; drop < 6; ++drop) {  // each output NULL in turn
      bb_play_plan_out o2{ob2.data(), oh.data(), oc.data(), ol.data(), osc.data(), os2.data()};
      if (drop == 0) o2.board = nullptr;
      if (drop == 1) o2.hand = nullptr;
      if (drop == 2) o2.combo = nullptr;
      if (drop == 3) o2.lines = nullptr;
      if (drop == 4) o2.score = nullptr;
      if (drop == 5) o2.status = nullptr;
      ok(bb_play_plan_pos(&pos, n, plan.data(), &o2, nullptr), "bb_play_plan_pos, one output NULL", nullptr);
      if (drop != 0) expect(ob2 == ob, "board again", drop);
      if (drop != 5) expect(os2 == os, "status again", drop);
    }
    int refills = 0, none = 0;
    for (int k = 0; k < n; ++k) {
      const int plies = os[k] & (int)BB_PLAY_PLIES;
      expect(!(os[k] & (int)BB_PLAY_ILLEGAL), "a plan of the search is legal", k);
      expect(plies == (plan[3 * k] >= 0) + (plan[3 * k + 1] >= 0) + (plan[3 * k + 2] >= 0), "plies played", k);
      expect(__builtin_popcount((oh[k] >> 18) & 7u) == plies && (oh[k] & 0x3FFFFu) == h[k], "used slots", k);
      refills += (os[k] & (int)BB_PLAY_REFILL) != 0;
      none += plies == 0;
      if (kAttempts[k / M][k % M] > 0) expect((os[k] & (int)BB_PLAY_REFILL) && plies == 3, "an accepted hand plays out", k);
    }
    expect(refills >= 20 && none >= 8, "plans of three plies and of none", refills);
  }

  // the handle form on fresh games (empty boards, combo 0) equals the stateless call on empty boards
  const bb_reward_cfg cfg = {1.0, 0.01, -1.0, -0.05, 0.02, 0.5, 0.001};
  const int ne = 3;
  bb_env* env = nullptr;
  ok(bb_create(ne, 0, &cfg, 0, &env), "bb_create", nullptr);
  ok(bb_reset(env, nullptr, nullptr), "bb_reset", env);
  std::vector<uint64_t> empty(ne, 0ull);
  std::vector<uint32_t> h1(ne * 4), h2(ne * 4);
  std::vector<int64_t> v1(ne * 4), v2(ne * 4);
  std::vector<int32_t> a1(ne * 4), a2(ne * 4);
  const bb_refill_values_out e1{h1.data(), v1.data(), a1.data()}, e2{h2.data(), v2.data(), a2.data()};
  ok(bb_refill_values(env, nullptr, &kW, 2, 4, 9, &e1, nullptr), "bb_refill_values", env);
  ok(bb_refill_values_pos(empty.data(), nullptr, nullptr, ne, &kW, 2, 4, 9, &e2, nullptr), "stateless twin", nullptr);
  expect(h1 == h2 && v1 == v2 && a1 == a2, "handle form", -1);

  // argument errors are reported, not crashes; n == 0 does nothing
  int64_t one = 7;
  const bb_refill_values_out o1{nullptr, &one, nullptr}, none{nullptr, nullptr, nullptr};
  if (bb_refill_values_pos(nullptr, nullptr, nullptr, 1, &kW, 1, 1, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, -1, &kW, 1, 1, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, nullptr, 1, 1, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 1, 1, 1, nullptr, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 1, 1, 1, &none, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 0, 1, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 4, 1, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 1, 0, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 1, &kW, 1, 1025, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values_pos(board.data(), nullptr, nullptr, 0, &kW, 1, 1, 1, &o1, nullptr) != BB_OK || one != 7 ||
      bb_refill_values(nullptr, nullptr, &kW, 1, 1, 1, &o1, nullptr) != BB_ERR_ARG ||
      bb_refill_values(env, nullptr, &kW, 1, 1, 1, &none, nullptr) != BB_ERR_ARG ||
      bb_play_plan_pos(nullptr, 1, nullptr, nullptr, nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks\n");
    g_fail = 1;
  }
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_refill_values and bb_play_plan_pos under sanitizers: %d boards x %d deals, hands equal the table\n", N, M);
  return 0;
}
