/*
 * draw_gate_model.c -- diagnostics (not product, not test): the iteration schedule of rollout_async_kernel's env
 * waves under a draw gate (csrc/bb_env.hip, BB_ASYNC_DGATE), on a replay of the bench workload.
 *
 * The bench workload (seeds 42 + i, the Philox random policy, auto-reset) is replayed on the C oracle for W warm-up
 * launches and one recorded launch of T steps.  Per env and step the replay records whether the move drew a new
 * hand, whether the shipped in-lane quick test (one slot: the fewest-anchor piece at its lowest anchor) accepts
 * attempt 1, and how many attempts _generate_new_pieces used.  Each group of 64 consecutive envs is then one env
 * wave, simulated iteration by iteration: moves, the gate's decision, draws (accept or post), poll, finalize.
 *
 * Cost weights (cycles): an iteration costs BASE, plus DRAW when the draw block runs.  BASE + DRAW is the parent's
 * measured iteration (tools/diag_async.py: 7,659); DRAW's share comes from the committed phase stamps
 * (profiles/r04/diag2_async_*.json: quick_post 3.1k and a quarter of move_draw 1.9k out of 9.1k stamped cycles =
 * 0.39, minus the move's accounting that stays = 0.34 -> 2.6k of 7.7k).
 * Search wait: a posted env is answered after SCALE * (u + 1 + LATER * p) cycles, u uniform in [0, 1) (the pick-up
 * by a search wave), p = 0, 1, 2 for a hand decided in attempts 1-4, 5-68, 69-100 (the quota schedule's passes).
 * SCALE and LATER are calibrated so that the parent schedule shows the parent build's measured blocked envs per
 * iteration and iterations per step (tools/diag_async.py blocked_envs_per_iter_per_wave, env_iters_per_step); the
 * gated schedules then use the same two values.
 * What the model leaves out: bursts of posts change the search waves' batch size, and fewer env-wave
 * instructions leave more issue slots to the search wave of the same SIMD.
 *
 *   gcc -O2 -fopenmp -o draw_gate_model tools/draw_gate_model.c -lm && ./draw_gate_model [N] [T] [W] [BLOCKED] [ITERS_PER_STEP] [BASE DRAW]
 */
#include <math.h>
#include <stdio.h>

struct Engine;
static void gen_hook(const struct Engine* e, int attempt, int ok);
#define BBO_GEN_HOOK(e, attempt, ok) gen_hook((const struct Engine*)(e), attempt, ok)
#include "../oracle/bb_oracle.c"

static uint64_t g_shape[NPIECES], g_anch[NPIECES];
static int g_offs[NPIECES][9], g_dtab[NPIECES][NPIECES];

static void init_bits(void) {
  init_pieces();
  for (int p = 0; p < NPIECES; ++p) {
    const Piece* pc = &g_pieces[p];
    uint64_t s = 0, a = 0;
    for (int k = 0; k < pc->n; ++k) {
      g_offs[p][k] = pc->dr[k] * 8 + pc->dc[k];
      s |= 1ull << g_offs[p][k];
    }
    for (int r = 0; r <= 8 - pc->h; ++r)
      for (int c = 0; c <= 8 - pc->w; ++c) a |= 1ull << (r * 8 + c);
    g_shape[p] = s;
    g_anch[p] = a;
  }
  for (int b = 0; b < NPIECES; ++b)
    for (int c = 0; c < NPIECES; ++c) {
      int seen[128] = {0}, cnt = 0;
      for (int i = 0; i < g_pieces[b].n; ++i)
        for (int j = 0; j < g_pieces[c].n; ++j) {
          const int d = g_offs[b][i] - g_offs[c][j] + 64;
          if (!seen[d]) seen[d] = 1, ++cnt;
        }
      g_dtab[b][c] = cnt;
    }
}

static uint64_t anchors_of(int p, uint64_t B) {
  uint64_t acc = 0;
  for (int k = 0; k < g_pieces[p].n; ++k) acc |= B >> g_offs[p][k];
  return g_anch[p] & ~acc;
}

static uint64_t clear_full(uint64_t B) {
  uint64_t r = B & (B >> 1), c = B & (B >> 8);
  r &= r >> 2, r &= r >> 4, r &= 0x0101010101010101ull;
  c &= c >> 16, c &= c >> 32, c &= 0xFFull;
  uint64_t rm = (r << 8) - r, cm = c | (c << 8);
  cm |= cm << 16, cm |= cm << 32;
  return B & ~(rm | cm);
}

/* the pair test of the in-lane quick test (bb_solver.h): the |D| bound, then the first leaf of each order */
static int pair_quick(uint64_t B1, int b, int c) {
  const uint64_t A2 = anchors_of(b, B1), A3 = anchors_of(c, B1);
  if (!(A2 | A3)) return 0;
  if (A2 && __builtin_popcountll(A3) > g_dtab[b][c]) return 1;
  if (A3 && __builtin_popcountll(A2) > g_dtab[b][c]) return 1;
  if (A2 && anchors_of(c, clear_full(B1 | (g_shape[b] << __builtin_ctzll(A2))))) return 1;
  if (A3 && anchors_of(b, clear_full(B1 | (g_shape[c] << __builtin_ctzll(A3))))) return 1;
  return 0;
}

/* BB_ASYNC_QPICK = 1, one slot: the hand's fewest-anchor piece (ties by slot) at its lowest anchor */
static int quick_accepts(uint64_t B, const int h[3]) {
  int f = -1, best = 65;
  for (int i = 0; i < 3; ++i) {
    const int c = __builtin_popcountll(anchors_of(h[i], B));
    if (c && c < best) best = c, f = i;
  }
  if (f < 0) return 0;
  const int b = f == 0 ? 1 : 0, c = f == 2 ? 1 : 2;
  const int p = __builtin_ctzll(anchors_of(h[f], B));
  return pair_quick(clear_full(B | (g_shape[h[f]] << p)), h[b], h[c]);
}

/* per env and step of the recorded launch: 0 no draw, 1 drawn and accepted in-lane, 1 + round when posted */
static uint8_t* g_rec;
static const Env* g_envs;
static int g_t = -1, g_T;

static void gen_hook(const struct Engine* ee, int attempt, int ok) {
  const Engine* e = (const Engine*)ee;
  if (g_t < 0 || grid_bits(&e->board) == 0) return; /* warm-up, or an episode reset's hand (drawn in finalize) */
  uint8_t* r = &g_rec[(size_t)((const Env*)ee - g_envs) * g_T + g_t];
  if (attempt == 0) {
    const int acc = quick_accepts(grid_bits(&e->board), e->hand);
    if (acc && !ok) fprintf(stderr, "quick test unsound\n"), exit(1);
    *r = acc ? 1 : 2;
  }
  if (*r >= 2) *r = (uint8_t)(2 + (attempt >= 4) + (attempt >= 68));
}

typedef struct {
  double iters, draw_runs, cyc, cyc_max, blocked, posts, bursts, gate_wait, draw_lanes;
} Res;

static double BASE = 5100.0, DRAW = 2600.0, IDLE = 300.0, LATER = 1.0;

static uint64_t g_lcg;
static double urand(void) {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_lcg >> 11) / 9007199254740992.0;
}

/* thr8: eighths of the runnable lanes that open the gate (0: no gate); lim: closed iterations that open it */
static Res simulate(int n, int T, int thr8, int lim, double scale) {
  Res R = {0};
  const int nw = n / 64;
  g_lcg = 12345;
  for (int w = 0; w < nw; ++w) {
    int st[64] = {0}, ph[64] = {0};
    double wake[64] = {0}, now = 0;
    int closed = 0;
    for (;;) {
      int left = 0, moved = 0, want = 0, run = 0, fin = 0;
      for (int l = 0; l < 64; ++l) left += st[l] < T;
      if (!left) break;
      for (int l = 0; l < 64; ++l) {
        R.blocked += ph[l] == 1;
        if (ph[l] == 0 && st[l] < T) ph[l] = g_rec[(size_t)(w * 64 + l) * T + st[l]] ? 3 : 2, ++moved;
        want += ph[l] == 3;
        run += ph[l] != 1 && st[l] < T;
      }
      const int open = !thr8 || thr8 * run <= 8 * want || closed >= lim || !moved;
      closed = (want && !open) ? closed + 1 : 0;
      const int ran = open && want;
      const double cost = BASE + (ran ? DRAW : 0.0);
      if (ran) {
        int posts = 0;
        for (int l = 0; l < 64; ++l)
          if (ph[l] == 3) {
            const int ev = g_rec[(size_t)(w * 64 + l) * T + st[l]];
            if (ev == 1) {
              ph[l] = 2;
            } else {
              ph[l] = 1, ++posts;
              wake[l] = now + 0.6 * cost + scale * (urand() + 1.0 + LATER * (ev - 2));
            }
          }
        R.draw_runs += 1, R.draw_lanes += want, R.posts += posts, R.bursts += posts > 0;
      } else {
        R.gate_wait += want;
      }
      for (int l = 0; l < 64; ++l) { /* the poll sits behind the move and the draw block: 0.6 of the iteration */
        if (ph[l] == 1 && wake[l] <= now + 0.6 * cost) ph[l] = 2;
        if (ph[l] == 2) ph[l] = 0, ++st[l], ++fin;
      }
      now += (moved || fin || ran) ? cost : IDLE;
      R.iters += 1;
    }
    R.cyc += now;
    if (now > R.cyc_max) R.cyc_max = now;
  }
  R.blocked /= R.iters;
  R.posts /= R.bursts > 0 ? R.bursts : 1;
  R.draw_lanes /= R.draw_runs > 0 ? R.draw_runs : 1;
  R.iters /= nw, R.draw_runs /= nw, R.cyc /= nw, R.gate_wait /= nw;
  return R;
}

int main(int argc, char** argv) {
  const int n = (argc > 1 ? atoi(argv[1]) : 8192) / 64 * 64;
  const int T = argc > 2 ? atoi(argv[2]) : 128;
  const int W = argc > 3 ? atoi(argv[3]) : 3;
  const double target = argc > 4 ? atof(argv[4]) : 8.40;
  const double target_ips = argc > 5 ? atof(argv[5]) : 1.383;
  if (argc > 7) BASE = atof(argv[6]), DRAW = atof(argv[7]);
  init_bits();
  uint64_t* seeds = malloc(sizeof(uint64_t) * n);
  for (int i = 0; i < n; ++i) seeds[i] = 42 + (uint64_t)i;
  bbo_vec* v = bbo_create(n, seeds, NULL, NULL, 1);
  bbo_reset(v, 1);
  uint64_t* m = malloc(sizeof(uint64_t) * 3 * n);
  int32_t* a = malloc(sizeof(int32_t) * n);
  bbo_state(v, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, m);
  bbo_random_actions(m, n, 0xB10C, 0, 0, a);
  g_envs = v->envs;
  g_T = T;
  g_rec = calloc((size_t)n * T, 1);
  if (W > 0) bbo_rollout(v, W * T, a, 0xB10C, 0, 0, NULL, NULL, NULL, NULL, NULL, 0);
  for (int t = 0; t < T; ++t) { /* one step per call: the hook files its records under the step */
    g_t = t;
    bbo_rollout(v, 1, a, 0xB10C, (uint64_t)(W * T + t), 0, NULL, NULL, NULL, NULL, NULL, 0);
  }
  size_t draws = 0, posted = 0;
  for (size_t k = 0; k < (size_t)n * T; ++k) draws += g_rec[k] > 0, posted += g_rec[k] > 1;
  printf("envs %d, T %d after %d warm-up launches: draws per env-step %.4f, posted share of draws %.4f\n", n, T, W,
         (double)draws / ((double)n * T), (double)posted / (double)draws);
  /* SCALE by bisection: the parent schedule's blocked envs per iteration = target; LATER (the weight of a later
   * pass) from a grid: the parent schedule's iterations per step closest to the measured figure */
  double scale = 0.0, best = 1e9, best_later = 0.0;
  for (int g = 0; g <= 20; ++g) {
    LATER = 0.1 * g;
    double lo = 0.0, hi = 200000.0;
    for (int k = 0; k < 30; ++k) {
      const double mid = 0.5 * (lo + hi);
      if (simulate(n, T, 0, 0, mid).blocked < target) lo = mid; else hi = mid;
    }
    const double err = fabs(simulate(n, T, 0, 0, 0.5 * (lo + hi)).iters / T - target_ips);
    if (err < best) best = err, best_later = LATER, scale = 0.5 * (lo + hi);
  }
  LATER = best_later;
  printf("weights: base %.0f + draw block %.0f cycles; search wait %.0f * (u + 1 + %.1f per later pass) cycles\n"
         "(parent schedule calibrated to blocked/iter %.2f, iterations per step %.3f)\n",
         BASE, DRAW, scale, LATER, target, target_ips);
  const Res P = simulate(n, T, 0, 0, scale);
  printf("%-22s %9s %9s %9s %9s %8s %8s %8s %8s %8s\n", "gate (eighths, limit)", "iter/step", "drawruns", "cyc mean",
         "cyc max", "vs par", "blocked", "post/bst", "lanes/run", "gatewait");
  static const int cfg[][2] = {{0, 0}, {4, 1}, {3, 2}, {4, 2}, {5, 2}, {6, 2}, {3, 3}, {4, 3}, {6, 3}, {4, 4}, {8, 2}};
  for (size_t c = 0; c < sizeof(cfg) / sizeof(cfg[0]); ++c) {
    const Res R = simulate(n, T, cfg[c][0], cfg[c][1], scale);
    char name[32];
    snprintf(name, sizeof name, cfg[c][0] ? "%d/8, %d" : "parent (no gate)", cfg[c][0], cfg[c][1]);
    printf("%-22s %9.4f %9.1f %9.0f %9.0f %8.4f %8.2f %8.2f %8.2f %8.1f\n", name, R.iters / T, R.draw_runs, R.cyc,
           R.cyc_max, R.cyc / P.cyc, R.blocked, R.posts, R.draw_lanes, R.gate_wait);
  }
  return 0;
}
