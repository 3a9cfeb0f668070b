// bb_lookahead.hip -- one-ply lookahead (gfx950): bb_afterstates / bb_greedy_actions of include/bbvec.h.
//
// The deterministic half of a step for all 192 actions of a position: what engine.py:326-346
// (can_place_piece) accepts, what engine.py:390-454 (make_move) does before it draws a new hand, and the
// reward of block_blast_env.py:148-193 for it.  Nothing here reads or writes env state beyond the four
// position columns, and no random number is drawn.
//
// Layout: one wave64 per (position, hand slot), lane = anchor cell, so lane l of slot p is flat action
// p*64 + l.  The slot's piece id is the same in every lane: its PieceRow is read through scalar loads from
// the kernel arguments (the whole 37-row table is passed by value: no table allocation, nothing to stage,
// and the launches stay graph-capturable), and no lane diverges from another on the piece.  A workgroup is
// the three waves of one position: the dense kernel's stores are 64 consecutive elements per wave and
// output, and the greedy kernel reduces (value, action) across each wave with shuffles and joins the three
// slots through 3 LDS records.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_env_internal.h"

namespace bb {

namespace {

constexpr int kLookBlock = 192;       // three waves: the three hand slots of one position
constexpr int64_t kLookMaxGrid = 1 << 15;  // more positions than this: the workgroups stride over them

struct LookTable {
  PieceRow row[kPieces];
};

// What one legal placement leads to (illegal: legal == false and the rest unspecified).
struct After {
  bool legal, dead, refill;
  uint64_t board;  // B' (after the clears)
  int ncells, lines, combo1, holes, centre, filled, mobility;
  int64_t gained;
};

// Lane `cell` of slot p: engine.py:326-346 (legal), 390-431 (place, clear, combo, score), then the
// mobility of the slots that stay unused (engine.py:348-362 valid_moves on the new board).
__device__ __forceinline__ After eval_action(const LookTable& t, uint64_t B, uint32_t hand, int combo, int p,
                                             int cell) {
  After a;
  const uint32_t used0 = hand_used(hand);
  const uint32_t id = hand_id(hand, p);
  const PieceRow& pr = t.row[id < (uint32_t)kPieces ? id : 0u];  // an id outside the table places nowhere
  a.legal = id < (uint32_t)kPieces && !hand_over(hand) && !((used0 >> p) & 1u) &&
            ((anchors_of(pr, B) >> cell) & 1ull);
  a.ncells = (int)ncells_of(pr);
  int rows, cols;
  a.board = clear_full(B | (pr.shape << cell), rows, cols);
  a.lines = rows + cols;
  a.combo1 = a.lines > 0 ? combo + 1 : 0;
  const int cm = a.lines < 4 ? a.lines : 4;
  const int streak = a.combo1 + 1 < 8 ? a.combo1 + 1 : 8;  // post-increment combo (engine.py:261)
  a.gained = a.lines > 0 ? a.ncells + (int64_t)(a.lines * 8 * 10) * cm * streak : (int64_t)a.ncells;
  const uint32_t used = used0 | (1u << p);
  a.refill = used == 7u;
  int mob = 0;
#pragma unroll
  for (int q = 0; q < kHand; ++q) {  // q and `used` are wave-uniform: no divergence
    const uint32_t idq = hand_id(hand, q);
    if (!((used >> q) & 1u) && idq < (uint32_t)kPieces) mob += __popcll(anchors_of(t.row[idq], a.board));
  }
  a.mobility = mob;
  a.dead = !a.refill && mob == 0;
  a.holes = count_holes(a.board);
  a.centre = __popcll(a.board & kCenter);
  a.filled = __popcll(a.board);
  return a;
}

// _calculate_reward of a legal move (block_blast_env.py:158-193) with game_over = dead: the same fp64
// operations in the same order as move_reward in bb_env.hip (restated here so that file stays untouched).
__device__ __forceinline__ double after_reward(const After& a, const bb_reward_cfg& cfg, double center_tenth,
                                               uint32_t prev) {
  const int cm = a.lines > 0 ? (a.lines < 4 ? a.lines : 4) : 1;
  double R = 0.0;
  R = __dadd_rn(R, __dmul_rn((double)a.ncells, cfg.block_placed));
  R = __dadd_rn(R, cfg.survival_bonus);
  if (a.lines > 0) {
    double lr = __dmul_rn((double)a.lines, cfg.line_clear_base);
    lr = __dmul_rn(lr, (double)cm);
    R = __dadd_rn(R, lr);
    if (cm > 1) R = __dadd_rn(R, __dmul_rn((double)(cm - 1), cfg.combo_multiplier_bonus));
  }
  if (a.dead) R = __dadd_rn(R, cfg.game_over_penalty);
  const int dh = a.holes - (int)(prev & 0xFFu);
  if (dh > 0) R = __dadd_rn(R, __dmul_rn((double)dh, cfg.hole_penalty));
  if (a.centre <= (int)(prev >> 8)) R = __dadd_rn(R, center_tenth);  // openness >= previous
  return R;
}

__device__ __forceinline__ uint32_t pack_aux(const After& a) {
  return 1u | ((uint32_t)a.dead << 1) | ((uint32_t)a.refill << 2) | ((uint32_t)a.lines << 8) |
         ((uint32_t)a.holes << 12) | ((uint32_t)a.centre << 19) | ((uint32_t)a.mobility << 24);
}

// The position columns are read at a wave-uniform index; readfirstlane tells the compiler so, which keeps the
// position in scalar registers and makes the piece-table reads scalar loads.
__device__ __forceinline__ uint32_t uniform32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  return ((uint64_t)uniform32((uint32_t)(x >> 32)) << 32) | uniform32((uint32_t)x);
}

struct LookPos {
  const uint64_t* board;
  const uint32_t* hand;
  const int32_t* combo;
  const uint16_t* prev;
};

__global__ void __launch_bounds__(kLookBlock)
afterstates_kernel(LookTable t, LookPos pos, int n, bb_reward_cfg cfg, double center_tenth, bb_afterstate_out out) {
  const int p = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // hand slot: one per wave
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const uint64_t B = uniform64(pos.board[i]);
    const uint32_t hand = uniform32(pos.hand[i]);
    const int combo = (int)uniform32(pos.combo ? (uint32_t)pos.combo[i] : 0u);
    const uint32_t prev = uniform32(pos.prev ? pos.prev[i] : 0u);
    const After a = eval_action(t, B, hand, combo, p, cell);
    const int64_t o = i * 192 + (int64_t)(p * 64 + cell);
    if (out.board) out.board[o] = a.legal ? a.board : B;
    if (out.reward_f64) out.reward_f64[o] = a.legal ? after_reward(a, cfg, center_tenth, prev) : -10.0;
    if (out.score_gained) out.score_gained[o] = a.legal ? (int32_t)a.gained : 0;
    if (out.aux) out.aux[o] = a.legal ? pack_aux(a) : 0u;
  }
}

// (value, action) order of the greedy choice: the larger value, then the lower action
__device__ __forceinline__ void take_better(int64_t& v, int& act, int64_t v2, int act2) {
  const bool better = v2 > v || (v2 == v && act2 < act);
  v = better ? v2 : v;
  act = better ? act2 : act;
}

__global__ void __launch_bounds__(kLookBlock)
greedy_kernel(LookTable t, LookPos pos, int n, bb_greedy_weights w, int32_t* __restrict__ action,
              int64_t* __restrict__ value) {
  __shared__ int64_t s_v[kHand];
  __shared__ int s_a[kHand];
  const int p = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const After a = eval_action(t, uniform64(pos.board[i]), uniform32(pos.hand[i]),
                                (int)uniform32(pos.combo ? (uint32_t)pos.combo[i] : 0u), p, cell);
    // an illegal lane carries (INT64_MIN, 0): every legal value is above INT64_MIN (|weight| < 2^31, every
    // feature < 2^15), so it never wins over a legal lane, and with no legal lane the result is action 0
    int64_t v = (int64_t)w.lines * a.lines + (int64_t)w.score * a.gained + (int64_t)w.holes * a.holes +
                (int64_t)w.filled * a.filled + (int64_t)w.centre * a.centre + (int64_t)w.mobility * a.mobility +
                (int64_t)w.dead * (int)a.dead + (int64_t)w.refill * (int)a.refill;
    v = a.legal ? v : INT64_MIN;
    int act = a.legal ? p * 64 + cell : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int64_t v2 = __shfl_xor(v, d, 64);
      const int act2 = __shfl_xor(act, d, 64);
      take_better(v, act, v2, act2);
    }
    if (cell == 0) {
      s_v[p] = v;
      s_a[p] = act;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      take_better(v, act, s_v[1], s_a[1]);
      take_better(v, act, s_v[2], s_a[2]);
      action[i] = act;
      if (value) value[i] = v;
    }
    __syncthreads();  // the records are rewritten by the workgroup's next position
  }
}

const LookTable& look_table() {
  static const LookTable t = [] {
    LookTable x;
    uint8_t dtab[kPieces * kPieces];
    build_piece_tables(x.row, dtab);
    return x;
  }();
  return t;
}

inline dim3 look_grid(int n) { return dim3((unsigned)((int64_t)n < kLookMaxGrid ? (int64_t)n : kLookMaxGrid)); }

}  // namespace

hipError_t launch_afterstates(const uint64_t* board, const uint32_t* hand, const int32_t* combo, const uint16_t* prev,
                              int n, const bb_reward_cfg& cfg, const bb_afterstate_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, prev};
  hipLaunchKernelGGL(afterstates_kernel, look_grid(n), dim3(kLookBlock), 0, s, look_table(), pos, n, cfg,
                     cfg.center_bonus * 0.1, out);
  return hipGetLastError();
}

hipError_t launch_greedy(const uint64_t* board, const uint32_t* hand, const int32_t* combo, const uint16_t* prev,
                         int n, const bb_greedy_weights& w, int32_t* action, int64_t* value, hipStream_t s) {
  const LookPos pos{board, hand, combo, prev};
  hipLaunchKernelGGL(greedy_kernel, look_grid(n), dim3(kLookBlock), 0, s, look_table(), pos, n, w, action, value);
  return hipGetLastError();
}

}  // namespace bb
