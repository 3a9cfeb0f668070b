// Sanitizer driver for the host backend's bb_snapshot_combo (csrc/bb_host.cpp).  TEST INFRASTRUCTURE: built by
// tests/test_distill_sanitize.py with -fsanitize=address,undefined.  Games are played with random legal moves
// (auto-reset on); after every step the combo column is copied into an exactly sized buffer and held to
// bb_get_state's, and the copied (board, hand, combo) positions go through bb_plan_values_pos, whose values with
// the score weight on read the combo.  Any sanitizer report aborts the process; a mismatch exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bbvec.h"

static void ok(int rc, const char* what, bb_env* env) {
  if (rc != BB_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, bb_last_error(env));
    exit(2);
  }
}

int main(void) {
  const bb_reward_cfg cfg = {1.0, 0.01, -1.0, -0.05, 0.02, 0.5, 0.001};
  const int n = 48, steps = 80;
  bb_env* env = nullptr;
  std::vector<uint64_t> seeds(n), raw(4 * (size_t)n);
  std::vector<uint8_t> has(n, 1);
  for (int i = 0; i < n; ++i) {
    seeds[i] = 700 + (uint64_t)i;
    ok(bb_pcg64_seed(seeds[i], &raw[4 * (size_t)i]), "bb_pcg64_seed", nullptr);
  }
  ok(bb_create(n, 0, &cfg, 1, &env), "bb_create", nullptr);
  ok(bb_seed(env, seeds.data(), has.data(), raw.data()), "bb_seed", env);
  ok(bb_reset(env, nullptr, nullptr), "bb_reset", env);
  std::vector<uint64_t> board(n), mb(3 * (size_t)n);
  std::vector<uint32_t> hand(n);
  std::vector<int32_t> act(n), combo(n), want(n);
  std::vector<float> rw(n);
  std::vector<uint8_t> tm(n);
  std::vector<int64_t> q((size_t)n * 192), q0((size_t)n * 192);
  const bb_greedy_weights w = {100, 1, -30, -2, 0, 1, -100000, 0};
  int fail = 0, nonzero = 0, combo_read = 0;
  for (int s = 0; s < steps; ++s) {
    ok(bb_obs(env, nullptr, nullptr, nullptr, mb.data(), nullptr), "bb_obs", env);
    ok(bb_random_actions(mb.data(), n, 0xB10C, (uint64_t)s, 0, act.data(), nullptr), "bb_random_actions", env);
    bb_step_out so{rw.data(), tm.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr};
    ok(bb_step(env, act.data(), &so, nullptr), "bb_step", env);
    ok(bb_snapshot(env, board.data(), hand.data(), nullptr, nullptr), "bb_snapshot", env);
    ok(bb_snapshot_combo(env, combo.data(), nullptr), "bb_snapshot_combo", env);
    bb_state_view sv{nullptr, nullptr, nullptr, want.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr};
    ok(bb_get_state(env, &sv), "bb_get_state", env);
    for (int i = 0; i < n; ++i) {
      if (combo[i] != want[i]) {
        fprintf(stderr, "MISMATCH combo at step %d env %d: %d != %d\n", s, i, combo[i], want[i]);
        fail = 1;
      }
      nonzero += combo[i] != 0;
    }
    if (s % 16 == 15) {  // the stored positions are searchable, and the combo column matters to the values
      const bb_positions with{board.data(), hand.data(), combo.data(), nullptr};
      const bb_positions without{board.data(), hand.data(), nullptr, nullptr};
      const bb_plan_values_out o{q.data(), nullptr, nullptr, nullptr}, o0{q0.data(), nullptr, nullptr, nullptr};
      ok(bb_plan_values_pos(&with, n, &w, 2, &o, nullptr), "bb_plan_values_pos", nullptr);
      ok(bb_plan_values_pos(&without, n, &w, 2, &o0, nullptr), "bb_plan_values_pos (combo 0)", nullptr);
      combo_read += q != q0;
    }
  }
  if (bb_snapshot_combo(nullptr, combo.data(), nullptr) != BB_ERR_ARG ||
      bb_snapshot_combo(env, nullptr, nullptr) != BB_OK) {
    fprintf(stderr, "argument checks\n");
    fail = 1;
  }
  if (nonzero == 0) {
    fprintf(stderr, "combo never left zero: the run shows nothing\n");
    fail = 1;
  }
  bb_destroy(env);
  if (fail) return 1;
  printf("bb_snapshot_combo under sanitizers: %d envs x %d steps equal bb_get_state (%d non-zero combos, %d of %d "
         "searches read them)\n", n, steps, nonzero, combo_read, steps / 16);
  return 0;
}
