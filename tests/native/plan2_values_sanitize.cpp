// Sanitizer driver for the host backend's two-hand decision (bb_plan2_values(_pos) and bb_plan2_work_bytes of
// csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by tests/test_plan2_values_sanitize.py with
// -fsanitize=address,undefined.  The positions of tests/native/values_ext_sanitize.cpp (a few random moves into a
// game, the crafted dead, finished and last-piece positions) with one row of twelve weights and one stream id per
// position in heap buffers of exactly n elements, the workspace in a heap buffer of exactly bb_plan2_work_bytes bytes
// (the call carves eight arrays out of it: an offset that is off is the error this is for) and every output in a heap
// buffer of exactly the size the call may write.  All five outputs are held to steps 2-6 restated here over
// bb_plan_values_ext_pos, bb_play_plan_pos and bb_refill_values_ext_pos; each output asked for alone (the others then
// live in the workspace) must equal the full call's; one shared row and the handle form are held to the _pos form.
// Any sanitizer report aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
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

template <class T>
static T* heap(size_t count) {
  T* p = (T*)malloc(sizeof(T) * (count ? count : 1));
  if (!p) exit(2);
  memset(p, 0x5A, sizeof(T) * count);
  return p;
}

// the five outputs of a call, each exactly as large as the call may write
struct Out {
  int n, k, m;
  int32_t *action, *cand, *status;
  int64_t *q2, *value;
  Out(int n_, int k_, int m_)
      : n(n_), k(k_), m(m_), action(heap<int32_t>(n_)), cand(heap<int32_t>((size_t)n_ * k_)),
        status(heap<int32_t>((size_t)n_ * k_)), q2(heap<int64_t>((size_t)n_ * 192)),
        value(heap<int64_t>((size_t)n_ * k_ * m_)) {}
  ~Out() {
    free(action);
    free(cand);
    free(status);
    free(q2);
    free(value);
  }
  bb_plan2_out all() const { return bb_plan2_out{action, q2, cand, status, value}; }
  bool same(const Out& o) const {
    return !memcmp(action, o.action, sizeof(int32_t) * n) && !memcmp(cand, o.cand, sizeof(int32_t) * n * k) &&
           !memcmp(status, o.status, sizeof(int32_t) * n * k) && !memcmp(q2, o.q2, sizeof(int64_t) * n * 192) &&
           !memcmp(value, o.value, sizeof(int64_t) * n * k * m);
  }
};

// steps 1-6 over the existing entry points, one position at a time
static void restate(const uint64_t* board, const uint32_t* hand, const int32_t* combo, const uint64_t* stream, int n,
                    const bb_eval_weights* rows, int64_t w_stride, int depth, int k, int m, uint64_t seed, Out& want) {
  for (int i = 0; i < n; ++i) {
    const bb_eval_weights* w = rows + i * w_stride;
    const bb_positions one{board + i, hand + i, combo + i, nullptr};
    std::vector<int64_t> q(192);
    std::vector<int32_t> rest(192);
    const bb_plan_values_out pv{q.data(), rest.data(), nullptr, nullptr};
    ok(bb_plan_values_ext_pos(&one, 1, w, 0, depth, &pv, nullptr), "bb_plan_values_ext_pos", nullptr);
    std::vector<int> order(192);
    for (int a = 0; a < 192; ++a) order[a] = a;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return q[a] > q[b]; });
    for (int a = 0; a < 192; ++a) want.q2[(size_t)i * 192 + a] = INT64_MIN;
    int64_t best = INT64_MIN;
    int best_a = 192;
    for (int r = 0; r < k; ++r) {
      const size_t c = (size_t)i * k + r;
      const int a = order[r];
      want.cand[c] = want.status[c] = -1;
      for (int j = 0; j < m; ++j) want.value[c * m + j] = 0;
      if (q[a] == INT64_MIN) continue;
      const int r2 = rest[a] & 0xFF, r3 = (rest[a] >> 8) & 0xFF;
      const int32_t plan[3] = {a, r2 == 0xFF ? -1 : r2, r3 == 0xFF ? -1 : r3};
      uint64_t lb;
      int32_t lc, ll, ls;
      int64_t lscore;
      const bb_play_plan_out po{&lb, nullptr, &lc, &ll, &lscore, &ls};
      ok(bb_play_plan_pos(&one, 1, plan, &po, nullptr), "bb_play_plan_pos", nullptr);
      want.cand[c] = a;
      want.status[c] = ls;
      int64_t x = (int64_t)m * q[a];
      if ((uint32_t)ls & BB_PLAY_REFILL) {
        const uint64_t sid = stream ? stream[i] : (uint64_t)i;
        const bb_refill_values_out ro{nullptr, want.value + c * m, nullptr};
        ok(bb_refill_values_ext_pos(&lb, &lc, &sid, 1, w, 0, depth, m, seed, &ro, nullptr), "bb_refill_values_ext_pos",
           nullptr);
        x = (int64_t)m * ((int64_t)w->base.lines * ll + (int64_t)w->base.score * lscore);
        for (int j = 0; j < m; ++j) x += want.value[c * m + j];
      }
      want.q2[(size_t)i * 192 + a] = x;
      if (x > best || (x == best && a < best_a)) best = x, best_a = a;
    }
    want.action[i] = best_a == 192 ? 0 : best_a;
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
  uint64_t* board = heap<uint64_t>(n);
  uint32_t* hand = heap<uint32_t>(n);
  int32_t* combo = heap<int32_t>(n);
  std::vector<uint64_t> mb(3 * (size_t)played);
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
  bb_state_view sv{board, hand, nullptr, combo, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ok(bb_get_state(env, &sv), "bb_get_state", env);
  expect(board[0] == 0, "fresh board", 0);

  // crafted: two free cells per row and column, never adjacent; SINGLE, DOMINO_H, (used) SQUARE_3x3
  uint64_t tight = ~0ull;
  for (int i = 0; i < 8; ++i) tight &= ~((1ull << (i * 8 + i)) | (1ull << (i * 8 + (i + 4) % 8)));
  const int kDead = played, kOver = played + 1, kLast = played + 2;
  board[kDead] = tight;
  hand[kDead] = 0u | (1u << 6) | (36u << 12) | (1u << 20);
  combo[kDead] = 0;
  board[kOver] = tight;
  hand[kOver] = 17u | (1u << 6) | (36u << 12) | (1u << 21);
  combo[kOver] = 0;
  board[kLast] = tight;  // one piece left: every first move is a refill
  hand[kLast] = 0u | (1u << 6) | (36u << 12) | (1u << 19) | (1u << 20);
  combo[kLast] = 9;
  const bb_positions pos{board, hand, combo, nullptr};

  // one row and one stream id per position, exactly n of each; every other row has its shape weights at 0
  bb_eval_weights* rows = heap<bb_eval_weights>((size_t)n);
  uint64_t* stream = heap<uint64_t>((size_t)n);
  for (int i = 0; i < n; ++i) {
    rows[i] = bb_eval_weights{{100 - 7 * i, 3 * i - 5, -30 + 11 * i, i - 2, 5 - i, 1 + i, -100000 + 2500 * i, 7 * i},
                              -3 + 2 * i, 4 + i, 2 + 3 * i, 25 - 9 * i};
    if (i & 1) rows[i].perimeter = rows[i].room3 = rows[i].room5 = rows[i].fits = 0;
    stream[i] = 1000 + (uint64_t)(i / 2);
  }

  int refills = 0, absent = 0;
  const int cases[3][3] = {{1, 192, 1}, {2, 4, 3}, {3, 3, 2}};  // depth, candidates, deals
  for (const auto& cs : cases) {
    const int depth = cs[0], k = cs[1], m = cs[2];
    const uint64_t seed = 0x9E3779B97F4A7C15ull * (uint64_t)depth;
    const int64_t bytes = bb_plan2_work_bytes(n, k, m);
    expect(bytes == (((int64_t)n * (192 * 12 + k * 28 + k * m * 8) + 7) & ~(int64_t)7), "bb_plan2_work_bytes", depth);
    char* work = heap<char>((size_t)bytes);  // exactly the bytes asked for
    Out got(n, k, m), want(n, k, m);
    const bb_plan2_out go = got.all();
    ok(bb_plan2_values_pos(&pos, stream, n, rows, 1, depth, k, m, seed, work, bytes, &go, nullptr),
       "bb_plan2_values_pos", nullptr);
    restate(board, hand, combo, stream, n, rows, 1, depth, k, m, seed, want);
    expect(got.same(want), "the five outputs against the restatement, depth", depth);
    for (int c = 0; c < n * k; ++c) {
      refills += got.status[c] >= 0 && ((uint32_t)got.status[c] & BB_PLAY_REFILL);
      absent += got.status[c] < 0;
    }
    expect(got.action[kOver] == 0 && got.cand[(size_t)kOver * k] == -1, "a finished game has no candidate", depth);

    // each output alone: the others live in the workspace
    for (int which = 0; which < 5; ++which) {
      Out solo(n, k, m);
      bb_plan2_out so{nullptr, nullptr, nullptr, nullptr, nullptr};
      if (which == 0) so.action = solo.action;
      if (which == 1) so.q2 = solo.q2;
      if (which == 2) so.cand = solo.cand;
      if (which == 3) so.status = solo.status;
      if (which == 4) so.value = solo.value;
      memset(work, 0x5A, (size_t)bytes);
      ok(bb_plan2_values_pos(&pos, stream, n, rows, 1, depth, k, m, seed, work, bytes, &so, nullptr),
         "bb_plan2_values_pos (one output)", nullptr);
      const bool same =
          which == 0   ? !memcmp(solo.action, got.action, sizeof(int32_t) * n)
          : which == 1 ? !memcmp(solo.q2, got.q2, sizeof(int64_t) * n * 192)
          : which == 2 ? !memcmp(solo.cand, got.cand, sizeof(int32_t) * n * k)
          : which == 3 ? !memcmp(solo.status, got.status, sizeof(int32_t) * n * k)
                       : !memcmp(solo.value, got.value, sizeof(int64_t) * n * k * m);
      expect(same, "an output asked for alone", which);
    }

    // one shared row in a buffer of exactly one row, NULL stream ids
    bb_eval_weights* shared = heap<bb_eval_weights>(1);
    *shared = rows[2];
    Out sg(n, k, m), sw(n, k, m);
    const bb_plan2_out sgo = sg.all();
    ok(bb_plan2_values_pos(&pos, nullptr, n, shared, 0, depth, k, m, seed, work, bytes, &sgo, nullptr),
       "bb_plan2_values_pos (shared row)", nullptr);
    restate(board, hand, combo, nullptr, n, shared, 0, depth, k, m, seed, sw);
    expect(sg.same(sw), "one shared row, stream id = i, depth", depth);
    free(shared);

    // the handle form on the live columns of the played games: the _pos form on their state, a smaller workspace
    const int64_t hbytes = bb_plan2_work_bytes(played, k, m);
    char* hwork = heap<char>((size_t)hbytes);
    Out hg(played, k, m), hw(played, k, m);
    const bb_plan2_out hgo = hg.all(), hwo = hw.all();
    ok(bb_plan2_values(env, stream, rows, 1, depth, k, m, seed, hwork, hbytes, &hgo, nullptr), "bb_plan2_values", env);
    ok(bb_plan2_values_pos(&pos, stream, played, rows, 1, depth, k, m, seed, hwork, hbytes, &hwo, nullptr),
       "bb_plan2_values_pos (played)", nullptr);
    expect(hg.same(hw), "the handle form against the _pos form, depth", depth);
    expect(bb_plan2_values(env, stream, rows, 1, depth, k, m, seed, hwork, hbytes - 8, &hgo, nullptr) == BB_ERR_ARG,
           "a workspace that is too small is refused", depth);
    free(hwork);
    free(work);
  }
  expect(refills >= 12 && absent >= 12, "refill leaves and absent candidates occur", refills);

  bb_destroy(env);
  free(rows);
  free(stream);
  free(board);
  free(hand);
  free(combo);
  if (g_fail) return 1;
  printf("plan2 values under sanitizers: %d positions at depth 1-3, consistent\n", n);
  return 0;
}
