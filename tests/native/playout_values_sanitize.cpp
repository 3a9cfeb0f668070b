// Sanitizer driver for the host backend's dealt playouts (bb_playout_values(_pos) of csrc/bb_host.cpp).  TEST
// INFRASTRUCTURE: built by tests/test_playout_values_sanitize.py with -fsanitize=address,undefined.  The boards of a few
// games some random moves in, the full board and a board with two free cells per row and column; one row of twelve
// weights, one combo and one stream id per board in heap buffers of exactly n elements, and every output in a heap
// buffer of exactly n * playouts elements.  All nine outputs are held to the definition restated here over
// bb_refill_values_ext_pos, bb_plan_actions_ext_pos and bb_play_plan_pos, one pair and one hand at a time; each output
// asked for alone must equal the full call's; one shared row with NULL combos and stream ids, and the handle form, are
// held to the _pos form.  Any sanitizer report aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

template <class T>
static T* heap(size_t count) {
  T* p = (T*)malloc(sizeof(T) * (count ? count : 1));
  if (!p) exit(2);
  memset(p, 0x5A, sizeof(T) * count);
  return p;
}

// the nine outputs of a call, each exactly as large as the call may write
struct Out {
  size_t k;
  int64_t *value, *score;
  int32_t *lines, *plies, *hands, *status, *combo;
  uint64_t* board;
  uint32_t* hand;
  Out(int n, int m)
      : k((size_t)n * m), value(heap<int64_t>(k)), score(heap<int64_t>(k)), lines(heap<int32_t>(k)),
        plies(heap<int32_t>(k)), hands(heap<int32_t>(k)), status(heap<int32_t>(k)), combo(heap<int32_t>(k)),
        board(heap<uint64_t>(k)), hand(heap<uint32_t>(k)) {}
  ~Out() {
    free(value), free(score), free(lines), free(plies), free(hands), free(status), free(combo), free(board), free(hand);
  }
  bb_playout_out all() const { return bb_playout_out{value, score, lines, plies, hands, status, board, combo, hand}; }
  const void* field(int which) const {
    const void* f[9] = {value, score, lines, plies, hands, status, board, combo, hand};
    return f[which];
  }
  static size_t width(int which) { return which < 2 || which == 6 ? 8 : 4; }
  bool same(const Out& o) const {
    for (int w = 0; w < 9; ++w)
      if (memcmp(field(w), o.field(w), width(w) * k)) return false;
    return true;
  }
};

// the definition over the existing entry points, one (board, playout) pair and one hand at a time
static void restate(const uint64_t* board, const int32_t* combo, const uint64_t* stream, int n,
                    const bb_eval_weights* rows, int64_t w_stride, int depth, int m, int hands, uint64_t seed,
                    Out& want) {
  std::vector<uint32_t> dealt(m);
  std::vector<int64_t> vals(m);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < m; ++j) {
      const bb_eval_weights* w = rows + i * w_stride;
      const uint64_t sid = stream ? stream[i] : (uint64_t)i;
      uint64_t B = board[i];
      int32_t cb = combo ? combo[i] : 0;
      int64_t moved = 0, score = 0, value = 0;
      int32_t lines = 0, plies = 0, searched = 0, status = 0;
      uint32_t last = 0;
      for (int h = 0; h < hands; ++h) {
        const bb_refill_values_out ro{dealt.data(), vals.data(), nullptr};
        ok(bb_refill_values_ext_pos(&B, &cb, &sid, 1, w, 0, depth, m, seed + (uint64_t)h, &ro, nullptr),
           "bb_refill_values_ext_pos", nullptr);
        last = dealt[j];
        searched = h + 1;
        int32_t action, plan[3];
        int64_t v;
        const bb_positions one{&B, &last, &cb, nullptr};
        const bb_plan_out po{&action, &v, plan, nullptr};
        ok(bb_plan_actions_ext_pos(&one, 1, w, 0, depth, &po, nullptr), "bb_plan_actions_ext_pos", nullptr);
        if (plan[0] < 0) {  // no legal first move
          expect(vals[j] == (int64_t)w->base.dead, "a hand without a first move is priced at dead", i);
          value = moved + (int64_t)w->base.dead;
          status = 0;
          break;
        }
        expect(vals[j] == v, "the two searches agree", i);
        value = moved + v;
        uint64_t nb;
        int32_t nc, ll, st;
        int64_t sc;
        const bb_play_plan_out pl{&nb, nullptr, &nc, &ll, &sc, &st};
        ok(bb_play_plan_pos(&one, 1, plan, &pl, nullptr), "bb_play_plan_pos", nullptr);
        B = nb, cb = nc, lines += ll, score += sc, plies += st & (int32_t)BB_PLAY_PLIES, status = st;
        if (!((uint32_t)st & BB_PLAY_REFILL)) break;
        moved += (int64_t)w->base.lines * ll + (int64_t)w->base.score * sc;
      }
      const size_t o = (size_t)i * m + j;
      want.value[o] = value, want.score[o] = score, want.lines[o] = lines, want.plies[o] = plies;
      want.hands[o] = searched, want.status[o] = status, want.board[o] = B, want.combo[o] = cb, want.hand[o] = last;
    }
}

int main(void) {
  const bb_reward_cfg cfg = {1.0, 0.01, -1.0, -0.05, 0.02, 0.5, 0.001};
  const int played = 5;
  const int n = played + 2;

  // boards 0 .. played-1: a game each, board i after 3*i random legal moves (0: the fresh board)
  bb_env* env = nullptr;
  std::vector<uint64_t> seeds(played), raw(4 * (size_t)played);
  std::vector<uint8_t> has(played, 1);
  for (int i = 0; i < played; ++i) {
    seeds[i] = 200 + (uint64_t)i;
    ok(bb_pcg64_seed(seeds[i], &raw[4 * (size_t)i]), "bb_pcg64_seed", nullptr);
  }
  ok(bb_create(played, 0, &cfg, 0, &env), "bb_create", nullptr);
  ok(bb_seed(env, seeds.data(), has.data(), raw.data()), "bb_seed", env);
  ok(bb_reset(env, nullptr, nullptr), "bb_reset", env);
  uint64_t* board = heap<uint64_t>(n);
  int32_t* combo = heap<int32_t>(n);
  std::vector<uint32_t> hand(n);
  std::vector<uint64_t> mb(3 * (size_t)played);
  std::vector<int32_t> act(played);
  std::vector<float> rw(played);
  std::vector<uint8_t> tm(played);
  for (int s = 0; s < 3 * (played - 1); ++s) {
    ok(bb_obs(env, nullptr, nullptr, nullptr, mb.data(), nullptr), "bb_obs", env);
    ok(bb_random_actions(mb.data(), played, 0xB10C, (uint64_t)s, 0, act.data(), nullptr), "bb_random_actions", env);
    for (int i = 0; i < played; ++i)
      if (s >= 3 * i) act[i] = -1;  // env i stops after 3*i moves: an invalid action changes nothing
    bb_step_out so{rw.data(), tm.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr};
    ok(bb_step(env, act.data(), &so, nullptr), "bb_step", env);
  }
  bb_state_view sv{board, hand.data(), nullptr, combo, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ok(bb_get_state(env, &sv), "bb_get_state", env);
  expect(board[0] == 0, "fresh board", 0);

  // crafted: the full board (nothing is ever legal), and two free cells per row and column, never adjacent (only
  // the single cell fits: most deals are refused, a dealt hand rarely has a first move)
  uint64_t tight = ~0ull;
  for (int i = 0; i < 8; ++i) tight &= ~((1ull << (i * 8 + i)) | (1ull << (i * 8 + (i + 4) % 8)));
  board[played] = ~0ull;
  combo[played] = 0;
  board[played + 1] = tight;
  combo[played + 1] = 3;

  // one row and one stream id per board, exactly n of each; every other row has its shape weights at 0
  bb_eval_weights* rows = heap<bb_eval_weights>((size_t)n);
  uint64_t* stream = heap<uint64_t>((size_t)n);
  for (int i = 0; i < n; ++i) {
    rows[i] = bb_eval_weights{{100 - 7 * i, 3 * i - 5, -30 + 11 * i, i - 2, 5 - i, 1 + i, -100000 + 2500 * i, 7 * i},
                              -3 + 2 * i, 4 + i, 2 + 3 * i, 25 - 9 * i};
    if (i & 1) rows[i].perimeter = rows[i].room3 = rows[i].room5 = rows[i].fits = 0;
    stream[i] = 1000 + (uint64_t)(i / 2);
  }

  int survived = 0, stopped = 0;
  const int cases[4][3] = {{1, 3, 2}, {2, 2, 3}, {3, 3, 3}, {3, 2, 1}};  // depth, playouts, hands
  for (const auto& cs : cases) {
    const int depth = cs[0], m = cs[1], hands = cs[2];
    const uint64_t seed = ~0ull - (uint64_t)(depth - 1);  // depth 1: the second hand's key wraps to 0
    Out got(n, m), want(n, m);
    const bb_playout_out go = got.all();
    ok(bb_playout_values_pos(board, combo, stream, n, rows, 1, depth, m, hands, seed, &go, nullptr),
       "bb_playout_values_pos", nullptr);
    restate(board, combo, stream, n, rows, 1, depth, m, hands, seed, want);
    expect(got.same(want), "the nine outputs against the restatement, depth", depth);
    for (size_t c = 0; c < got.k; ++c) {
      survived += ((uint32_t)got.status[c] & BB_PLAY_REFILL) != 0;
      stopped += got.status[c] == 0;
    }
    for (int j = 0; j < m; ++j)
      expect(got.status[(size_t)played * m + j] == 0 && got.hands[(size_t)played * m + j] == 1 &&
                 got.value[(size_t)played * m + j] == rows[played].base.dead && got.board[(size_t)played * m + j] == ~0ull,
             "the full board has no first move", j);

    // each output alone, in a buffer of its own exact size
    for (int which = 0; which < 9; ++which) {
      Out solo(n, m);
      bb_playout_out so{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      if (which == 0) so.value = solo.value;
      if (which == 1) so.score = solo.score;
      if (which == 2) so.lines = solo.lines;
      if (which == 3) so.plies = solo.plies;
      if (which == 4) so.hands = solo.hands;
      if (which == 5) so.status = solo.status;
      if (which == 6) so.board = solo.board;
      if (which == 7) so.combo = solo.combo;
      if (which == 8) so.hand = solo.hand;
      ok(bb_playout_values_pos(board, combo, stream, n, rows, 1, depth, m, hands, seed, &so, nullptr),
         "bb_playout_values_pos (one output)", nullptr);
      expect(!memcmp(solo.field(which), got.field(which), Out::width(which) * got.k), "an output asked for alone", which);
    }

    // one shared row in a buffer of exactly one row, NULL combos and stream ids
    bb_eval_weights* shared = heap<bb_eval_weights>(1);
    *shared = rows[2];
    Out sg(n, m), sw(n, m);
    const bb_playout_out sgo = sg.all();
    ok(bb_playout_values_pos(board, nullptr, nullptr, n, shared, 0, depth, m, hands, seed, &sgo, nullptr),
       "bb_playout_values_pos (shared row)", nullptr);
    restate(board, nullptr, nullptr, n, shared, 0, depth, m, hands, seed, sw);
    expect(sg.same(sw), "one shared row, combo 0, stream id = i, depth", depth);
    free(shared);

    // the handle form on the live columns of the played games: the _pos form on their state
    Out hg(played, m), hw(played, m);
    const bb_playout_out hgo = hg.all(), hwo = hw.all();
    ok(bb_playout_values(env, stream, rows, 1, depth, m, hands, seed, &hgo, nullptr), "bb_playout_values", env);
    ok(bb_playout_values_pos(board, combo, stream, played, rows, 1, depth, m, hands, seed, &hwo, nullptr),
       "bb_playout_values_pos (played)", nullptr);
    expect(hg.same(hw), "the handle form against the _pos form, depth", depth);
    expect(bb_playout_values(env, stream, rows, 1, depth, m, 257, seed, &hgo, nullptr) == BB_ERR_ARG,
           "too many hands are refused", depth);
  }
  expect(survived >= 10 && stopped >= 10, "survivors and hands without a first move occur", survived);

  bb_destroy(env);
  free(rows);
  free(stream);
  free(board);
  free(combo);
  if (g_fail) return 1;
  printf("playout values under sanitizers: %d boards at depth 1-3, consistent\n", n);
  return 0;
}
