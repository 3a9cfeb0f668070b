// Sanitizer driver for the host backend's per-action values and dealt next-hand values with the shape terms
// (bb_plan_values_ext(_pos) and bb_refill_values_ext(_pos) of csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by
// tests/test_values_ext_sanitize.py with -fsanitize=address,undefined.  The positions of
// tests/native/eval_terms_sanitize.cpp (a few random moves into a game, the crafted dead, finished and last-piece
// positions), searched at depth 3 with one row of twelve weights per position in a heap buffer of exactly n rows (an
// off-by-one row read is the error this is for: the neighbouring row is checked to give other values), with one shared
// row in a buffer of exactly one row, and through the handle; every output in a heap buffer of exactly the size the
// call may write.  max_a q is held to bb_plan_actions_ext_pos, a dealt hand's value to bb_plan_actions_ext_pos on
// that hand, and rows whose shape weights are 0 to bb_plan_values_pos / bb_refill_values_pos.  Any sanitizer report
// aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
  T* p = (T*)malloc(sizeof(T) * count);
  if (!p) exit(2);
  memset(p, 0x5A, sizeof(T) * count);
  return p;
}

// the four outputs of a plan-values call, each exactly [n][192] / [n][3] on the heap
struct Values {
  int n;
  int64_t* q;
  int32_t *rest, *leaves;
  uint64_t* safe;
  explicit Values(int n_)
      : n(n_), q(heap<int64_t>(192 * (size_t)n_)), rest(heap<int32_t>(192 * (size_t)n_)),
        leaves(heap<int32_t>(192 * (size_t)n_)), safe(heap<uint64_t>(3 * (size_t)n_)) {}
  ~Values() {
    free(q);
    free(rest);
    free(leaves);
    free(safe);
  }
  bb_plan_values_out out() const { return bb_plan_values_out{q, rest, leaves, safe}; }
  bool same_row(int i, const Values& o, int j) const {
    return !memcmp(q + 192 * (size_t)i, o.q + 192 * (size_t)j, 192 * sizeof(int64_t)) &&
           !memcmp(rest + 192 * (size_t)i, o.rest + 192 * (size_t)j, 192 * sizeof(int32_t)) &&
           !memcmp(leaves + 192 * (size_t)i, o.leaves + 192 * (size_t)j, 192 * sizeof(int32_t)) &&
           !memcmp(safe + 3 * (size_t)i, o.safe + 3 * (size_t)j, 3 * sizeof(uint64_t));
  }
};

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

  // one row per position, all different, all four shape weights set; exactly n rows
  bb_eval_weights* rows = heap<bb_eval_weights>((size_t)n);
  for (int i = 0; i < n; ++i)
    rows[i] = bb_eval_weights{{100 - 37 * i, 3 * i - 5, -30 + 11 * i, i - 2, 5 - i, 1 + i, -100000 + 25000 * i, 7 * i},
                              -3 + 2 * i, 4 + i, 2 + 3 * i, 25 - 9 * i};
  rows[n - 1] = bb_eval_weights{{INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX},
                                INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX};

  // ---- per-action values: the batch under its own rows
  Values all(n);
  const bb_plan_values_out ao = all.out();
  ok(bb_plan_values_ext_pos(&pos, n, rows, 1, 3, &ao, nullptr), "bb_plan_values_ext_pos", nullptr);
  std::vector<int32_t> ea(n), el(n);
  std::vector<int64_t> ev(n);
  const bb_plan_out eo{ea.data(), ev.data(), nullptr, el.data()};
  ok(bb_plan_actions_ext_pos(&pos, n, rows, 1, 3, &eo, nullptr), "bb_plan_actions_ext_pos", nullptr);

  int differ = 0;
  for (int i = 0; i < n; ++i) {
    const bb_positions one{board.data() + i, hand.data() + i, combo.data() + i, nullptr};
    bb_eval_weights* shared = heap<bb_eval_weights>(1);
    *shared = rows[i];
    Values u(1), nb(1), z(1), p(1);
    const bb_plan_values_out uo = u.out(), no = nb.out(), zo = z.out(), po = p.out();
    ok(bb_plan_values_ext_pos(&one, 1, shared, 0, 3, &uo, nullptr), "bb_plan_values_ext_pos (shared row)", nullptr);
    expect(all.same_row(i, u, 0), "own row against the shared row", i);
    // max_a q, its lowest arg-max and the sum of leaves are the search's
    int64_t best = INT64_MIN;
    int arg = 0, leaves = 0;
    for (int a = 0; a < 192; ++a) {
      if (u.q[a] > best) best = u.q[a], arg = a;
      leaves += u.leaves[a];
    }
    expect(best == ev[i] && leaves == el[i] && (el[i] == 0 || arg == ea[i]), "max q / arg-max / leaves", i);
    // the neighbouring row would have given other values: the check above can tell an off-by-one
    if (i + 1 < n) {
      *shared = rows[i + 1];
      ok(bb_plan_values_ext_pos(&one, 1, shared, 0, 3, &no, nullptr), "bb_plan_values_ext_pos (next row)", nullptr);
      differ += memcmp(nb.q, u.q, 192 * sizeof(int64_t)) != 0;
      expect(!memcmp(nb.leaves, u.leaves, 192 * sizeof(int32_t)) && !memcmp(nb.safe, u.safe, 3 * sizeof(uint64_t)),
             "leaves and safe do not depend on the row", i);
    }
    // the shape weights at 0: the eight-weight values, output for output
    *shared = rows[i];
    shared->perimeter = shared->room3 = shared->room5 = shared->fits = 0;
    ok(bb_plan_values_ext_pos(&one, 1, shared, 0, 3, &zo, nullptr), "bb_plan_values_ext_pos (zero shape)", nullptr);
    ok(bb_plan_values_pos(&one, 1, &rows[i].base, 3, &po, nullptr), "bb_plan_values_pos", nullptr);
    expect(z.same_row(0, p, 0), "zero shape weights", i);
    free(shared);
    if (i == 0) expect(leaves > 50000, "fresh board: the largest tree", i);
    if (i == kDead) expect(leaves == 16, "dead: 16 sequences of one move", i);
    if (i == kOver) expect(best == INT64_MIN && leaves == 0 && u.rest[0] == -1, "game over: nothing legal", i);
    if (i == kLast) expect(leaves == 16 && u.rest[arg] == 0xFFFF, "last piece: every move is a refill", i);
  }
  expect(differ >= played, "neighbouring rows give other values", -1);

  // each output alone (the other three NULL), safe alone at depth 3 (searched at depth 2), and n == 0
  {
    Values o(n);
    const bb_plan_values_out qo{o.q, nullptr, nullptr, nullptr}, so{nullptr, nullptr, nullptr, o.safe};
    ok(bb_plan_values_ext_pos(&pos, n, rows, 1, 3, &qo, nullptr), "q alone", nullptr);
    ok(bb_plan_values_ext_pos(&pos, n, rows, 1, 3, &so, nullptr), "safe alone", nullptr);
    expect(!memcmp(o.q, all.q, 192 * sizeof(int64_t) * (size_t)n), "q alone", -1);
    expect(!memcmp(o.safe, all.safe, 3 * sizeof(uint64_t) * (size_t)n), "safe alone", -1);
    ok(bb_plan_values_ext_pos(&pos, 0, rows, 1, 3, &qo, nullptr), "n = 0", nullptr);
  }

  // the handle form on the played positions: num_envs rows, again exactly sized, then one shared row
  bb_eval_weights* hrows = heap<bb_eval_weights>((size_t)played);
  for (int i = 0; i < played; ++i) hrows[i] = rows[i];
  {
    Values h(played);
    const bb_plan_values_out ho = h.out();
    ok(bb_plan_values_ext(env, hrows, 1, 3, &ho, nullptr), "bb_plan_values_ext", env);
    for (int i = 0; i < played; ++i) expect(h.same_row(i, all, i), "handle values", i);
    ok(bb_plan_values_ext(env, hrows, 0, 3, &ho, nullptr), "bb_plan_values_ext (shared row)", env);
    expect(h.same_row(0, all, 0), "handle values, shared row", 0);
  }

  // ---- dealt next-hand values: m deals per board, every board under its own row; exactly [n][m] outputs
  const int m = 3;
  const uint64_t seed = 0x5EED;
  uint64_t* stream = heap<uint64_t>((size_t)n);
  for (int i = 0; i < n; ++i) stream[i] = 40 + (uint64_t)(i / 2);  // shared in pairs
  uint32_t* rh = heap<uint32_t>((size_t)n * m);
  int64_t* rv = heap<int64_t>((size_t)n * m);
  int32_t* ra = heap<int32_t>((size_t)n * m);
  const bb_refill_values_out ro{rh, rv, ra};
  ok(bb_refill_values_ext_pos(board.data(), combo.data(), stream, n, rows, 1, 3, m, seed, &ro, nullptr),
     "bb_refill_values_ext_pos", nullptr);
  uint32_t* bh = heap<uint32_t>((size_t)n * m);
  int32_t* ba = heap<int32_t>((size_t)n * m);
  const bb_refill_values_out bo{bh, nullptr, ba};
  ok(bb_refill_values_pos(board.data(), combo.data(), stream, n, &rows[0].base, 3, m, seed, &bo, nullptr),
     "bb_refill_values_pos", nullptr);
  expect(!memcmp(rh, bh, sizeof(uint32_t) * (size_t)n * m) && !memcmp(ra, ba, sizeof(int32_t) * (size_t)n * m),
         "hand and attempts are the eight-weight call's", -1);
  int rdiffer = 0, dealt_dead = 0;
  for (int i = 0; i < n; ++i) {
    bb_eval_weights* shared = heap<bb_eval_weights>(1);
    *shared = rows[i];
    int64_t* v1 = heap<int64_t>((size_t)m);
    const bb_refill_values_out o1{nullptr, v1, nullptr};
    ok(bb_refill_values_ext_pos(board.data() + i, combo.data() + i, stream + i, 1, shared, 0, 3, m, seed, &o1, nullptr),
       "bb_refill_values_ext_pos (shared row)", nullptr);
    expect(!memcmp(v1, rv + (size_t)i * m, sizeof(int64_t) * m), "own row against the shared row (refill)", i);
    for (int j = 0; j < m; ++j) {  // the value is the search's on the dealt hand
      const bb_positions one{board.data() + i, rh + (size_t)i * m + j, combo.data() + i, nullptr};
      int32_t a = -7, l = -7;
      int64_t v = 5;
      const bb_plan_out uo{&a, &v, nullptr, &l};
      ok(bb_plan_actions_ext_pos(&one, 1, shared, 0, 3, &uo, nullptr), "bb_plan_actions_ext_pos (dealt hand)", nullptr);
      expect(rv[(size_t)i * m + j] == (l ? v : (int64_t)rows[i].base.dead), "dealt hand's value", i);
      dealt_dead += l == 0;
    }
    if (i + 1 < n) {
      *shared = rows[i + 1];
      ok(bb_refill_values_ext_pos(board.data() + i, combo.data() + i, stream + i, 1, shared, 0, 3, m, seed, &o1,
                                  nullptr),
         "bb_refill_values_ext_pos (next row)", nullptr);
      rdiffer += memcmp(v1, rv + (size_t)i * m, sizeof(int64_t) * m) != 0;
    }
    *shared = rows[i];
    shared->perimeter = shared->room3 = shared->room5 = shared->fits = 0;
    int64_t* v0 = heap<int64_t>((size_t)m);
    const bb_refill_values_out z1{nullptr, v1, nullptr}, z0{nullptr, v0, nullptr};
    ok(bb_refill_values_ext_pos(board.data() + i, combo.data() + i, stream + i, 1, shared, 0, 3, m, seed, &z1, nullptr),
       "bb_refill_values_ext_pos (zero shape)", nullptr);
    ok(bb_refill_values_pos(board.data() + i, combo.data() + i, stream + i, 1, &rows[i].base, 3, m, seed, &z0, nullptr),
       "bb_refill_values_pos (one board)", nullptr);
    expect(!memcmp(v1, v0, sizeof(int64_t) * m), "zero shape weights (refill)", i);
    free(v0);
    free(v1);
    free(shared);
  }
  expect(rdiffer >= played, "neighbouring rows give other values (refill)", -1);
  expect(dealt_dead > 0, "the tight board is dealt hands without a first move", -1);
  // NULL combo and stream, n == 0, and the handle form
  {
    int64_t* v = heap<int64_t>((size_t)played * m);
    int64_t* w = heap<int64_t>((size_t)played * m);
    const bb_refill_values_out ho{nullptr, v, nullptr}, po{nullptr, w, nullptr};
    ok(bb_refill_values_ext(env, nullptr, hrows, 1, 3, m, seed, &ho, nullptr), "bb_refill_values_ext", env);
    ok(bb_refill_values_ext_pos(board.data(), combo.data(), nullptr, played, hrows, 1, 3, m, seed, &po, nullptr),
       "bb_refill_values_ext_pos (played)", nullptr);
    expect(!memcmp(v, w, sizeof(int64_t) * (size_t)played * m), "handle refill values", -1);
    ok(bb_refill_values_ext_pos(board.data(), nullptr, nullptr, 0, hrows, 1, 3, m, seed, &po, nullptr), "n = 0 (refill)",
       nullptr);
    free(w);
    free(v);
  }

  // argument errors are reported, not crashes
  if (bb_plan_values_ext_pos(&pos, n, nullptr, 1, 3, &ao, nullptr) != BB_ERR_ARG ||
      bb_plan_values_ext_pos(&pos, -1, rows, 1, 3, &ao, nullptr) != BB_ERR_ARG ||
      bb_plan_values_ext_pos(&pos, n, rows, 2, 3, &ao, nullptr) != BB_ERR_ARG ||
      bb_plan_values_ext_pos(&pos, n, rows, 1, 4, &ao, nullptr) != BB_ERR_ARG ||
      bb_plan_values_ext_pos(&pos, n, rows, 1, 3, nullptr, nullptr) != BB_ERR_ARG ||
      bb_plan_values_ext(env, nullptr, 1, 3, &ao, nullptr) != BB_ERR_ARG ||
      bb_plan_values_ext(env, hrows, 12, 3, &ao, nullptr) != BB_ERR_ARG ||
      bb_refill_values_ext_pos(nullptr, nullptr, nullptr, n, rows, 1, 3, m, seed, &ro, nullptr) != BB_ERR_ARG ||
      bb_refill_values_ext_pos(board.data(), nullptr, nullptr, n, nullptr, 1, 3, m, seed, &ro, nullptr) != BB_ERR_ARG ||
      bb_refill_values_ext_pos(board.data(), nullptr, nullptr, n, rows, -1, 3, m, seed, &ro, nullptr) != BB_ERR_ARG ||
      bb_refill_values_ext_pos(board.data(), nullptr, nullptr, n, rows, 1, 0, m, seed, &ro, nullptr) != BB_ERR_ARG ||
      bb_refill_values_ext_pos(board.data(), nullptr, nullptr, n, rows, 1, 3, 0, seed, &ro, nullptr) != BB_ERR_ARG ||
      bb_refill_values_ext(env, nullptr, hrows, 2, 3, m, seed, &ro, nullptr) != BB_ERR_ARG) {
    fprintf(stderr, "argument checks\n");
    g_fail = 1;
  }
  free(ba);
  free(bh);
  free(ra);
  free(rv);
  free(rh);
  free(stream);
  free(hrows);
  free(rows);
  bb_destroy(env);
  if (g_fail) return 1;
  printf("bb_plan_values_ext / bb_refill_values_ext under sanitizers: %d positions at depth 3, consistent\n", n);
  return 0;
}
