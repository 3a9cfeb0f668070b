// bb_lookahead.hip -- one-ply lookahead (gfx950): bb_afterstates / bb_greedy_actions(_each) of include/bbvec.h.
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
#include "bb_look_rules.h"

namespace bb {

namespace {

constexpr int kLookBlock = 192;       // three waves: the three hand slots of one position
constexpr int64_t kLookMaxGrid = 1 << 15;  // more positions than this: the workgroups stride over them

struct LookTable {
  PieceRow row[kPieces];
};

// Lane `cell` of slot p: engine.py:326-346 (legal), 390-431 (place, clear, combo, score), then the
// mobility of the slots that stay unused (engine.py:348-362 valid_moves on the new board).  After, its
// reward, aux word and value terms are the shared ones of bb_rules.h.
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
  a.combo1 = combo_after(a.lines, combo);
  a.gained = score_gained(a.ncells, a.lines, a.combo1);
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

// position i of the columns (i is wave-uniform), in scalar registers; a NULL combo column reads as 0
struct Position {
  uint64_t B;
  uint32_t hand;
  int combo;
};
__device__ __forceinline__ Position load_position(const LookPos& pos, int64_t i) {
  return Position{uniform64(pos.board[i]), uniform32(pos.hand[i]),
                  (int)uniform32(pos.combo ? (uint32_t)pos.combo[i] : 0u)};
}

__global__ void __launch_bounds__(kLookBlock)
afterstates_kernel(LookTable t, LookPos pos, int n, bb_reward_cfg cfg, double center_tenth, bb_afterstate_out out) {
  const int p = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // hand slot: one per wave
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);
    const uint32_t prev = uniform32(pos.prev ? pos.prev[i] : 0u);
    const After a = eval_action(t, P.B, P.hand, P.combo, p, cell);
    const int64_t o = i * 192 + (int64_t)(p * 64 + cell);
    if (out.board) out.board[o] = a.legal ? a.board : P.B;
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
    const Position P = load_position(pos, i);
    const After a = eval_action(t, P.B, P.hand, P.combo, p, cell);
    // an illegal lane carries (INT64_MIN, 0): every legal value is above INT64_MIN (|weight| < 2^31, every
    // feature < 2^15), so it never wins over a legal lane, and with no legal lane the result is action 0
    int64_t v = a.legal ? move_terms(w, a) + state_terms(w, a) : INT64_MIN;
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

// ---------------------------------------------------------------------------
// One row of weights per position (bbvec.h bb_greedy_actions_each / bb_plan_actions_each): greedy_kernel and
// plan_kernel with w = rows[i].  They are kernels of their own, not a template over the two above, so that the
// uniform kernels' code objects stay instruction for instruction what DESIGN.md measured (a shared body changed
// their scalar code).  The row is read inside the position loop -- a workgroup that strides past the grid cap meets
// another row at every position -- at the wave-uniform index i and, like the position, told to be uniform: eight
// scalar loads, the row in scalar registers.
// ---------------------------------------------------------------------------
static_assert(sizeof(bb_greedy_weights) == 8 * sizeof(int32_t), "a weight row is eight int32");
__device__ __forceinline__ bb_greedy_weights load_weights(const bb_greedy_weights* __restrict__ rows, int64_t i) {
  const int32_t* r = reinterpret_cast<const int32_t*>(rows + i);
  bb_greedy_weights w;
  w.lines = (int32_t)uniform32((uint32_t)r[0]);
  w.score = (int32_t)uniform32((uint32_t)r[1]);
  w.holes = (int32_t)uniform32((uint32_t)r[2]);
  w.filled = (int32_t)uniform32((uint32_t)r[3]);
  w.centre = (int32_t)uniform32((uint32_t)r[4]);
  w.mobility = (int32_t)uniform32((uint32_t)r[5]);
  w.dead = (int32_t)uniform32((uint32_t)r[6]);
  w.refill = (int32_t)uniform32((uint32_t)r[7]);
  return w;
}

__global__ void __launch_bounds__(kLookBlock)
greedy_each_kernel(LookTable t, LookPos pos, int n, const bb_greedy_weights* __restrict__ rows,
                   int32_t* __restrict__ action, int64_t* __restrict__ value) {
  __shared__ int64_t s_v[kHand];
  __shared__ int s_a[kHand];
  const int p = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);
    const bb_greedy_weights w = load_weights(rows, i);
    const After a = eval_action(t, P.B, P.hand, P.combo, p, cell);
    int64_t v = a.legal ? move_terms(w, a) + state_terms(w, a) : INT64_MIN;  // as greedy_kernel
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

// ---------------------------------------------------------------------------
// Full-hand lookahead (bbvec.h bb_plan_actions): the exhaustive search over every order and placement of the
// hand's unused pieces, up to `depth` plies, fused into one launch.
//
// One workgroup of four waves per position.
//   ply 1: wave p < 3 takes hand slot p, lane = anchor cell (as the one-ply kernels).  A legal afterstate that
//          ends its sequence (depth 1, refill or dead) is scored on the spot; the others are compacted by ballot
//          / prefix popcount into an LDS list of at most 192 records.
//   ply 2: the four waves take the records round-robin.  A record is wave-uniform (read back through
//          readfirstlane into scalar registers); for each slot still unused, lane = ply-2 cell.
//   ply 3: every legal, unfinished ply-2 lane loops over the set bits of its own anchor mask for the last piece
//          (board, partial sum and combo stay in the lane's registers).  The alternative -- walk those lanes
//          with a ballot, broadcast each one's board with readlane and evaluate the third piece for all 64 cells
//          at once, position in scalar registers -- was 26-36% slower at depth 3 (profiles/r08/plan/ab;
//          tools/patches/r08_plan_ply3_broadcast.diff).  The ply-2 list of a position (up to 24,576 entries)
//          never exists.
// Every lane keeps the best (value, key) it has seen, key = a1 << 16 | a2 << 8 | a3 with 0xFF for a ply not
// played: the larger value wins, then the lower key, which is the lexicographic order of (a1, a2, a3) because
// no maximal sequence is a prefix of another.  The lanes are joined by shuffles and the waves through four LDS
// records.  Trip bounds: <= 192 records, 3 slots, 64 mask bits.  No atomics, no inline assembly.
// ---------------------------------------------------------------------------
constexpr int kPlanWaves = 4;
constexpr int kPlanBlock = 64 * kPlanWaves;
constexpr int kPlanRecords = 192;            // the legal ply-1 afterstates of one position
constexpr int64_t kPlanMaxGrid = 1 << 14;    // more positions than this: the workgroups stride over them
constexpr uint32_t kPlanNoKey = 0xFFFFFFFFu;  // no maximal sequence seen

struct PlanRecord {
  uint64_t board;  // B' of the ply-1 move
  int64_t sum;     // w.lines * lines + w.score * score_gained so far
  int32_t combo;   // combo'
  int32_t action;  // a1
};

// (value, key) order of the plan choice: the larger value, then the lower key
__device__ __forceinline__ void take_plan(int64_t& v, uint32_t& key, int64_t v2, uint32_t key2) {
  const bool better = v2 > v || (v2 == v && key2 < key);
  v = better ? v2 : v;
  key = better ? key2 : key;
}

// ---- the search body shared by plan_kernel and plan_values_kernel ----

// Ply 1, evaluation: wave p < 3 takes hand slot p, lane = anchor cell.  `open`: legal and not the end of its
// sequence (goes to the record list); `closed`: legal and the end (depth 1, refill or dead).  Wave 3 gets a zeroed
// afterstate and neither flag: left indeterminate there, `a` costs each kernel 12 VGPRs (65 / 69 against 53 / 57).
struct Ply1 {
  After a;
  bool open, closed;
};
__device__ __forceinline__ Ply1 plan_ply1(const LookTable& t, const Position& P, int depth, int wave, int cell) {
  Ply1 r{};
  if (wave < kHand) {
    r.a = eval_action(t, P.B, P.hand, P.combo, wave, cell);
    const bool end1 = depth == 1 || r.a.refill || r.a.dead;
    r.open = r.a.legal && !end1;
    r.closed = r.a.legal && end1;
  }
  return r;
}

// Ply 1, compaction: the open lanes of waves 0..2 become the records s_rec[0..total), in action order (ballot,
// prefix popcount).  Returns total <= kPlanRecords; both barriers have passed.  The kernels call this after the
// lanes that are not open have used their afterstate (scored themselves, filled their staging entry): from here
// on only an open lane's board, move terms and combo' are needed, so nothing else of it is live across the barriers.
template <class W>  // bb_greedy_weights, or bb_eval_weights (plan_ext_kernel): move_terms / state_terms of bb_rules.h
__device__ __forceinline__ int plan_compact(PlanRecord* s_rec, int* s_cnt, const W& w, const Ply1& p1, int wave,
                                            int cell) {
  const uint64_t open_mask = __ballot(p1.open);
  if (wave < kHand && cell == 0) s_cnt[wave] = __popcll(open_mask);
  __syncthreads();
  const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2];
  const int total = __builtin_amdgcn_readfirstlane(c0 + c1 + c2);  // <= 192
  if (p1.open) {
    const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(open_mask >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)open_mask, 0u));
    const int slot = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + before;  // < total <= kPlanRecords
    s_rec[slot] = PlanRecord{p1.a.board, move_terms(w, p1.a), p1.a.combo1, wave * 64 + cell};
  }
  __syncthreads();
  return total;
}

// Plies 2 and 3 below one record, by one wave: the record is wave-uniform (read back through readfirstlane into
// scalar registers); for each slot still unused, lane = ply-2 cell, and ply 3 is the per-lane loop.  Every leaf
// goes into the lane's (best, best_key, leaves).  kPerFirstMove = false (plan_kernel): the key carries a1,
// key = a1 << 16 | a2 << 8 | a3, and `alive` is not touched.  true (plan_values_kernel): key = a2 << 8 | a3, and
// `alive` is set by a leaf that is not dead.  Returns a1, the record's action (< 192).
template <bool kPerFirstMove, class W>
__device__ __forceinline__ int plan_record_turn(const LookTable& t, const PlanRecord& rec, uint32_t hand,
                                                const W& w, int depth, int cell, int64_t& best,
                                                uint32_t& best_key, int& leaves, bool& alive) {
  const uint64_t B1 = uniform64(rec.board);
  const int64_t sum1 = (int64_t)uniform64((uint64_t)rec.sum);
  const int combo1 = (int)uniform32((uint32_t)rec.combo);
  const int act1 = (int)uniform32((uint32_t)rec.action);
  const uint32_t hand1 = hand_use(hand, act1 >> 6);
#pragma unroll 1
  for (int q = 0; q < kHand; ++q) {
    if ((hand_used(hand1) >> q) & 1u) continue;  // wave-uniform
    const After a2 = eval_action(t, B1, hand1, combo1, q, cell);
    const bool end2 = depth == 2 || a2.refill || a2.dead;
    const int64_t sum2 = sum1 + move_terms(w, a2);
    const uint32_t key2 = (kPerFirstMove ? 0u : (uint32_t)act1 << 16) | ((uint32_t)(q * 64 + cell) << 8);
    if (a2.legal && end2) {
      take_plan(best, best_key, sum2 + state_terms(w, a2), key2 | 0xFFu);
      ++leaves;
      if (kPerFirstMove) alive |= !a2.dead;
    }
    // ply 3.  An unfinished ply-2 afterstate means the hand was whole: one slot is left, its piece fits
    // somewhere and placing it ends the sequence (refill, never dead).  Each such lane walks the set bits of its
    // own ply-3 anchor mask; the lanes' trip counts differ, the bound is the 64 bits.
    if (a2.legal && !end2) {
      const uint32_t hand2 = hand_use(hand1, q);
      const int q3 = __ffs((int)(~hand_used(hand2) & 7u)) - 1;  // wave-uniform; >= 0 here
      const uint32_t id3 = hand_id(hand2, q3);
      uint64_t m3 = anchors_of(t.row[id3 < (uint32_t)kPieces ? id3 : 0u], a2.board);  // != 0: not dead
      if (kPerFirstMove) alive = true;
      for (int it = 0; it < 64 && m3 != 0ull; ++it) {
        const int c3 = __ffsll((unsigned long long)m3) - 1;
        m3 &= m3 - 1ull;
        const After a3 = eval_action(t, a2.board, hand2, a2.combo1, q3, c3);  // legal by construction
        take_plan(best, best_key, sum2 + move_terms(w, a3) + state_terms(w, a3), key2 | (uint32_t)(q3 * 64 + c3));
        ++leaves;
      }
    }
  }
  return act1;
}

// the wave's lanes joined: every lane ends with the wave's best (value, key) and its leaf count
__device__ __forceinline__ void plan_wave_join(int64_t& best, uint32_t& best_key, int& leaves) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t v2 = __shfl_xor(best, d, 64);
    const uint32_t k2 = (uint32_t)__shfl_xor((int)best_key, d, 64);
    take_plan(best, best_key, v2, k2);
    leaves += __shfl_xor(leaves, d, 64);
  }
}

__global__ void __launch_bounds__(kPlanBlock)
plan_kernel(LookTable t, LookPos pos, int n, bb_greedy_weights w, int depth, bb_plan_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_key[kPlanWaves];
  __shared__ int s_leaves[kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);
    int64_t best = INT64_MIN;  // below every legal value (see greedy_kernel)
    uint32_t best_key = kPlanNoKey;
    int leaves = 0;
    bool unused = false;  // `alive` is plan_values_kernel's

    // ---- ply 1: a closed lane scores itself, then the open ones are compacted
    const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
    if (ply1.closed) {
      best = move_terms(w, ply1.a) + state_terms(w, ply1.a);
      best_key = ((uint32_t)(wave * 64 + cell) << 16) | 0xFFFFu;
      leaves = 1;
    }
    const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);

    // ---- ply 2 (and 3): one record per wave and turn, the accumulators kept across the records
    for (int r = wave; r < total; r += kPlanWaves)
      plan_record_turn<false>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, unused);

    // ---- join the lanes, then the waves
    plan_wave_join(best, best_key, leaves);
    if (cell == 0) {
      s_v[wave] = best;
      s_key[wave] = best_key;
      s_leaves[wave] = leaves;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < kPlanWaves; ++k) {
        take_plan(best, best_key, s_v[k], s_key[k]);
        leaves += s_leaves[k];
      }
      const bool found = best_key != kPlanNoKey;
      const int p1 = (int)(best_key >> 16), p2 = (int)((best_key >> 8) & 0xFFu), p3 = (int)(best_key & 0xFFu);
      out.action[i] = found ? p1 : 0;
      if (out.value) out.value[i] = best;
      if (out.plan) {
        out.plan[i * 3 + 0] = found ? p1 : -1;
        out.plan[i * 3 + 1] = found && p2 != 0xFF ? p2 : -1;
        out.plan[i * 3 + 2] = found && p3 != 0xFF ? p3 : -1;
      }
      if (out.leaves) out.leaves[i] = leaves;
    }
    // no barrier here: the next position's first LDS writes (s_cnt, s_rec) touch nothing thread 0 still reads,
    // and its s_v / s_key / s_leaves writes come after two more barriers that thread 0 has to reach first
  }
}

// plan_kernel with w = rows[i] (see greedy_each_kernel): the same search body, the same LDS, barriers and join
__global__ void __launch_bounds__(kPlanBlock)
plan_each_kernel(LookTable t, LookPos pos, int n, const bb_greedy_weights* __restrict__ rows, int depth,
                 bb_plan_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_key[kPlanWaves];
  __shared__ int s_leaves[kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);
    const bb_greedy_weights w = load_weights(rows, i);
    int64_t best = INT64_MIN;
    uint32_t best_key = kPlanNoKey;
    int leaves = 0;
    bool unused = false;

    const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
    if (ply1.closed) {
      best = move_terms(w, ply1.a) + state_terms(w, ply1.a);
      best_key = ((uint32_t)(wave * 64 + cell) << 16) | 0xFFFFu;
      leaves = 1;
    }
    const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);

    for (int r = wave; r < total; r += kPlanWaves)
      plan_record_turn<false>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, unused);

    plan_wave_join(best, best_key, leaves);
    if (cell == 0) {
      s_v[wave] = best;
      s_key[wave] = best_key;
      s_leaves[wave] = leaves;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < kPlanWaves; ++k) {
        take_plan(best, best_key, s_v[k], s_key[k]);
        leaves += s_leaves[k];
      }
      const bool found = best_key != kPlanNoKey;
      const int p1 = (int)(best_key >> 16), p2 = (int)((best_key >> 8) & 0xFFu), p3 = (int)(best_key & 0xFFu);
      out.action[i] = found ? p1 : 0;
      if (out.value) out.value[i] = best;
      if (out.plan) {
        out.plan[i * 3 + 0] = found ? p1 : -1;
        out.plan[i * 3 + 1] = found && p2 != 0xFF ? p2 : -1;
        out.plan[i * 3 + 2] = found && p3 != 0xFF ? p3 : -1;
      }
      if (out.leaves) out.leaves[i] = leaves;
    }
    // no barrier here, as in plan_kernel: thread 0 reads only s_v / s_key / s_leaves, which the next position
    // writes after two more barriers; its row is in this wave's own registers
  }
}

// ---------------------------------------------------------------------------
// The search with the shape terms (bbvec.h bb_plan_actions_ext): plan_each_kernel under bb_eval_weights.  The same
// search body -- plan_compact and plan_record_turn instantiated for the twelve-int row, whose state_terms adds
// shape_terms of the leaf's board (bb_rules.h) -- the same LDS, barriers and join.  The row of position i is
// rows[i * w_stride], w_stride 0 (one row for all) or 1; it is read inside the position loop into scalar registers,
// so the tests "is this term's weight 0" are scalar branches, the same for the whole workgroup, and a term that is
// switched off costs a position nothing else.  fits is the dear one: a leaf on whose board the 3x3 square fits
// pays four bar tests, any other leaf 36 anchor boards of two to three ands each.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bb_eval_weights load_eval_weights(const bb_eval_weights* __restrict__ rows, int64_t i) {
  const int32_t* r = reinterpret_cast<const int32_t*>(rows + i);
  bb_eval_weights w;
  w.base.lines = (int32_t)uniform32((uint32_t)r[0]);
  w.base.score = (int32_t)uniform32((uint32_t)r[1]);
  w.base.holes = (int32_t)uniform32((uint32_t)r[2]);
  w.base.filled = (int32_t)uniform32((uint32_t)r[3]);
  w.base.centre = (int32_t)uniform32((uint32_t)r[4]);
  w.base.mobility = (int32_t)uniform32((uint32_t)r[5]);
  w.base.dead = (int32_t)uniform32((uint32_t)r[6]);
  w.base.refill = (int32_t)uniform32((uint32_t)r[7]);
  w.perimeter = (int32_t)uniform32((uint32_t)r[8]);
  w.room3 = (int32_t)uniform32((uint32_t)r[9]);
  w.room5 = (int32_t)uniform32((uint32_t)r[10]);
  w.fits = (int32_t)uniform32((uint32_t)r[11]);
  return w;
}

// plan_kernel's search of one position up to the wave join, under either weight type (plan_ext_kernel's two sides)
template <class W>
__device__ __forceinline__ void plan_search(const LookTable& t, const Position& P, const W& w, int depth, int wave,
                                            int cell, PlanRecord* s_rec, int* s_cnt, int64_t& best,
                                            uint32_t& best_key, int& leaves) {
  bool unused = false;  // `alive` is plan_values_kernel's
  const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
  if (ply1.closed) {
    best = move_terms(w, ply1.a) + state_terms(w, ply1.a);
    best_key = ((uint32_t)(wave * 64 + cell) << 16) | 0xFFFFu;
    leaves = 1;
  }
  const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);
  for (int r = wave; r < total; r += kPlanWaves)
    plan_record_turn<false>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, unused);
}

__global__ void __launch_bounds__(kPlanBlock)
plan_ext_kernel(LookTable t, LookPos pos, int n, const bb_eval_weights* __restrict__ rows, int64_t w_stride,
                int depth, bb_plan_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_key[kPlanWaves];
  __shared__ int s_leaves[kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);
    const bb_eval_weights w = load_eval_weights(rows, i * w_stride);
    const bool shaped = (w.perimeter | w.room3 | w.room5 | w.fits) != 0;  // scalar: one answer for the workgroup
    int64_t best = INT64_MIN;
    uint32_t best_key = kPlanNoKey;
    int leaves = 0;

    // a row with the four shape weights 0 takes plan_each_kernel's search, the eight-weight instantiation: the shape
    // code, skipped branch by branch, still lengthened the twelve-weight leaf loop ("Shape terms").
    // The barriers inside are met by the whole workgroup on either side: every wave read the same row.
    if (shaped)
      plan_search(t, P, w, depth, wave, cell, s_rec, s_cnt, best, best_key, leaves);
    else
      plan_search(t, P, w.base, depth, wave, cell, s_rec, s_cnt, best, best_key, leaves);

    plan_wave_join(best, best_key, leaves);
    if (cell == 0) {
      s_v[wave] = best;
      s_key[wave] = best_key;
      s_leaves[wave] = leaves;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < kPlanWaves; ++k) {
        take_plan(best, best_key, s_v[k], s_key[k]);
        leaves += s_leaves[k];
      }
      const bool found = best_key != kPlanNoKey;
      const int p1 = (int)(best_key >> 16), p2 = (int)((best_key >> 8) & 0xFFu), p3 = (int)(best_key & 0xFFu);
      out.action[i] = found ? p1 : 0;
      if (out.value) out.value[i] = best;
      if (out.plan) {
        out.plan[i * 3 + 0] = found ? p1 : -1;
        out.plan[i * 3 + 1] = found && p2 != 0xFF ? p2 : -1;
        out.plan[i * 3 + 2] = found && p3 != 0xFF ? p3 : -1;
      }
      if (out.leaves) out.leaves[i] = leaves;
    }
    // no barrier here, as in plan_kernel
  }
}

// ---------------------------------------------------------------------------
// The shape terms of a board column (bbvec.h bb_board_terms): one lane per board, board_terms of bb_rules.h, four
// int32 per board.  Above the grid cap the lanes stride.  No LDS, no atomics, no inline assembly.
// ---------------------------------------------------------------------------
constexpr int kTermsBlock = 256;
constexpr int64_t kTermsMaxGrid = 1 << 10;

__global__ void __launch_bounds__(kTermsBlock)
board_terms_kernel(const uint64_t* __restrict__ board, int n, int32_t* __restrict__ terms) {
  const int64_t stride = (int64_t)gridDim.x * kTermsBlock;
  for (int64_t i = (int64_t)blockIdx.x * kTermsBlock + threadIdx.x; i < (int64_t)n; i += stride) {
    int32_t v[4];
    board_terms(board[i], v);
    terms[i * 4 + 0] = v[0];
    terms[i * 4 + 1] = v[1];
    terms[i * 4 + 2] = v[2];
    terms[i * 4 + 3] = v[3];
  }
}

// ---------------------------------------------------------------------------
// Per-action full-hand values (bbvec.h bb_plan_values): plan_kernel's search with the maximum kept per first move.
//
// Same layout and the same search body as plan_kernel.  A record is one first move, so the best (value,
// key16 = a2 << 8 | a3), the leaf count and "some leaf is not dead" start fresh with every record and are joined
// across the wave (shuffles, one ballot) at the end of the record's turn.  Results are staged in LDS arrays
// indexed by action: a ply-1 lane fills its own action's entry when the action is illegal or ends its sequence
// there, lane 0 of the owning wave fills an open record's.  After one barrier threads 0..191 store the rows, 64
// consecutive elements per wave and output, and waves 0..2 make the three safe words by ballot.
//
// Unlike plan_kernel this one needs a barrier at the end of a position: the next position's ply-1 lanes write
// the staging arrays as their first act, while slower waves may still be reading them for the stores.
// ---------------------------------------------------------------------------
constexpr uint32_t kRestNone = 0xFFFFu;  // rest of a sequence that ends at ply 1

__global__ void __launch_bounds__(kPlanBlock)
plan_values_kernel(LookTable t, LookPos pos, int n, bb_greedy_weights w, int depth, bb_plan_values_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_q[BB_ACTIONS];
  __shared__ int32_t s_rest[BB_ACTIONS];
  __shared__ int32_t s_leaves[BB_ACTIONS];
  __shared__ uint8_t s_safe[BB_ACTIONS];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);

    // ---- ply 1: threadIdx.x is the action of waves 0..2.  A lane that is not open (illegal, or a sequence of
    // one move) fills its staging entry, then the open ones are compacted
    const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
    if (wave < kHand && !ply1.open) {
      s_q[threadIdx.x] = ply1.closed ? move_terms(w, ply1.a) + state_terms(w, ply1.a) : INT64_MIN;
      s_rest[threadIdx.x] = ply1.closed ? (int32_t)kRestNone : -1;
      s_leaves[threadIdx.x] = ply1.closed ? 1 : 0;
      s_safe[threadIdx.x] = (uint8_t)(ply1.closed && !ply1.a.dead);
    }
    const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);

    // ---- ply 2 (and 3): one record = one first move per wave and turn, the accumulators fresh for each
    for (int r = wave; r < total; r += kPlanWaves) {
      int64_t best = INT64_MIN;  // below every legal value (see greedy_kernel)
      uint32_t best_key = kPlanNoKey;
      int leaves = 0;
      bool alive = false;  // a leaf with dead == 0
      const int act1 = plan_record_turn<true>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, alive);
      // the record's turn ends: join the lanes (the whole wave is here, the loops of the turn are wave-uniform)
      plan_wave_join(best, best_key, leaves);
      const bool any_alive = __ballot(alive) != 0ull;
      if (cell == 0) {  // an open record has a leaf: its afterstate is not dead.  act1 indexes the staging arrays
        s_q[act1] = best;
        s_rest[act1] = (int32_t)(((best_key >> 8) & 0xFFu) | ((best_key & 0xFFu) << 8));
        s_leaves[act1] = leaves;
        s_safe[act1] = (uint8_t)any_alive;
      }
    }
    __syncthreads();

    // ---- store the rows: thread = action
    if (wave < kHand) {
      const int64_t o = i * BB_ACTIONS + (int64_t)threadIdx.x;
      if (out.q) out.q[o] = s_q[threadIdx.x];
      if (out.rest) out.rest[o] = s_rest[threadIdx.x];
      if (out.leaves) out.leaves[o] = s_leaves[threadIdx.x];
      const uint64_t safe = __ballot(s_safe[threadIdx.x] != 0);
      if (out.safe && cell == 0) out.safe[i * kHand + wave] = safe;
    }
    __syncthreads();  // the staging arrays are rewritten by the first lanes to reach the workgroup's next position
  }
}

// plan_values_kernel's search of one position up to the barrier before the stores, restated as a template over the
// weight type for plan_values_ext_kernel's two sides: the ply-1 staging, the compaction, the record turns with their
// fresh accumulators, the wave join and the ballot.  Both barriers of plan_compact are inside; the stores and the two
// barriers around them are the kernel's.  plan_values_kernel keeps its own text, as plan_kernel does beside
// plan_search: called through this template it no longer compiled to its listing (54 -> 57 VGPRs;
// profiles/values_ext/isa_compare.txt).
template <class W>
__device__ __forceinline__ void plan_values_search(const LookTable& t, const Position& P, const W& w, int depth,
                                                   int wave, int cell, PlanRecord* s_rec, int* s_cnt, int64_t* s_q,
                                                   int32_t* s_rest, int32_t* s_leaves, uint8_t* s_safe) {
  // ---- ply 1: threadIdx.x is the action of waves 0..2.  A lane that is not open (illegal, or a sequence of
  // one move) fills its staging entry, then the open ones are compacted
  const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
  if (wave < kHand && !ply1.open) {
    s_q[threadIdx.x] = ply1.closed ? move_terms(w, ply1.a) + state_terms(w, ply1.a) : INT64_MIN;
    s_rest[threadIdx.x] = ply1.closed ? (int32_t)kRestNone : -1;
    s_leaves[threadIdx.x] = ply1.closed ? 1 : 0;
    s_safe[threadIdx.x] = (uint8_t)(ply1.closed && !ply1.a.dead);
  }
  const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);

  // ---- ply 2 (and 3): one record = one first move per wave and turn, the accumulators fresh for each
  for (int r = wave; r < total; r += kPlanWaves) {
    int64_t best = INT64_MIN;  // below every legal value (see greedy_kernel)
    uint32_t best_key = kPlanNoKey;
    int leaves = 0;
    bool alive = false;  // a leaf with dead == 0
    const int act1 = plan_record_turn<true>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, alive);
    // the record's turn ends: join the lanes (the whole wave is here, the loops of the turn are wave-uniform)
    plan_wave_join(best, best_key, leaves);
    const bool any_alive = __ballot(alive) != 0ull;
    if (cell == 0) {  // an open record has a leaf: its afterstate is not dead.  act1 indexes the staging arrays
      s_q[act1] = best;
      s_rest[act1] = (int32_t)(((best_key >> 8) & 0xFFu) | ((best_key & 0xFFu) << 8));
      s_leaves[act1] = leaves;
      s_safe[act1] = (uint8_t)any_alive;
    }
  }
}

// plan_values_kernel under rows of bb_eval_weights (bbvec.h bb_plan_values_ext): position i takes
// rows[i * w_stride], w_stride 0 or 1, read inside the position loop into scalar registers.  Two sides, as
// plan_ext_kernel: a row whose four shape weights are 0 takes the eight-weight instantiation under w.base, any
// other the twelve-weight one.  Every wave reads the same row, so the branch is the workgroup's, and both sides
// meet the same barriers (the two of plan_compact); the barrier before the stores and the one at the end of a
// position are outside the branch.  The same LDS, trip bounds and grid cap as plan_values_kernel.
__global__ void __launch_bounds__(kPlanBlock)
plan_values_ext_kernel(LookTable t, LookPos pos, int n, const bb_eval_weights* __restrict__ rows, int64_t w_stride,
                       int depth, bb_plan_values_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_q[BB_ACTIONS];
  __shared__ int32_t s_rest[BB_ACTIONS];
  __shared__ int32_t s_leaves[BB_ACTIONS];
  __shared__ uint8_t s_safe[BB_ACTIONS];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const Position P = load_position(pos, i);
    const bb_eval_weights w = load_eval_weights(rows, i * w_stride);
    const bool shaped = (w.perimeter | w.room3 | w.room5 | w.fits) != 0;  // scalar: one answer for the workgroup
    if (shaped)
      plan_values_search(t, P, w, depth, wave, cell, s_rec, s_cnt, s_q, s_rest, s_leaves, s_safe);
    else
      plan_values_search(t, P, w.base, depth, wave, cell, s_rec, s_cnt, s_q, s_rest, s_leaves, s_safe);
    __syncthreads();

    // ---- store the rows: thread = action
    if (wave < kHand) {
      const int64_t o = i * BB_ACTIONS + (int64_t)threadIdx.x;
      if (out.q) out.q[o] = s_q[threadIdx.x];
      if (out.rest) out.rest[o] = s_rest[threadIdx.x];
      if (out.leaves) out.leaves[o] = s_leaves[threadIdx.x];
      const uint64_t safe = __ballot(s_safe[threadIdx.x] != 0);
      if (out.safe && cell == 0) out.safe[i * kHand + wave] = safe;
    }
    __syncthreads();  // the staging arrays are rewritten by the first lanes to reach the workgroup's next position
  }
}

// ---------------------------------------------------------------------------
// The hand-safe mask alone (bbvec.h bb_safe_mask): plan_values_kernel's safe words of depth >= 2 by an existence
// search.  No values, so no weights, no combo, no record list: after first move a, can the rest of the hand still
// be placed in some order?
//
// One wave64 per position, four positions per workgroup, the waves independent: no LDS, no barrier, so nothing
// of one position can be overwritten by the next one a wave strides to.  The wave takes the three hand slots in
// turn (a used slot is skipped by a wave-uniform branch), lane = anchor cell, the position in scalar registers and
// the rows of the pieces that stay in the hand read through scalar loads.  A legal lane answers for its own first
// move: nothing left -- safe; one piece left -- one anchors_of; two pieces left -- trip k of its loop tries the
// k-th lowest anchor of either order (both leaves computed and or-ed, as pair_quick_bf does, so trip 0 is each
// order's first leaf, which settles an open board) and the lane leaves at its first success.  Trip bound: 64 (an
// anchor mask has 64 bits; both orders advance together).  The words are made by ballot, the "some action is safe"
// of mode 1 is an or of three scalar words, and lanes 0..2 store one word each.  No atomics, no inline assembly.
// ---------------------------------------------------------------------------
constexpr int kSafeWaves = 4;                // positions per workgroup
constexpr int kSafeBlock = 64 * kSafeWaves;
constexpr int64_t kSafeMaxGrid = 1 << 15;    // more than 4 * this many positions: the waves stride over them

// anchors of the piece in hand slot q on board X; a piece id outside the table places nowhere
__device__ __forceinline__ uint64_t slot_anchors(const LookTable& t, uint32_t hand, int q, uint64_t X) {
  const uint32_t id = hand_id(hand, q);
  return id < (uint32_t)kPieces ? anchors_of(t.row[id], X) : 0ull;
}

__global__ void __launch_bounds__(kSafeBlock)
safe_mask_kernel(LookTable t, LookPos pos, int n, int mode, uint64_t* __restrict__ mask) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  const int64_t stride = (int64_t)gridDim.x * kSafeWaves;
  for (int64_t i = (int64_t)blockIdx.x * kSafeWaves + wave; i < (int64_t)n; i += stride) {  // i is wave-uniform
    const uint64_t B = uniform64(pos.board[i]);
    const uint32_t hand = uniform32(pos.hand[i]);
    const uint32_t used0 = hand_used(hand);
    uint64_t safe_w[kHand] = {0ull, 0ull, 0ull}, legal_w[kHand] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int p = 0; p < kHand; ++p) {
      const uint32_t id = hand_id(hand, p);
      if (hand_over(hand) || ((used0 >> p) & 1u) || id >= (uint32_t)kPieces) continue;  // wave-uniform
      const PieceRow& pr = t.row[id];
      const bool legal = (anchors_of(pr, B) >> cell) & 1ull;
      const uint32_t left = ~(used0 | (1u << p)) & 7u;  // the slots that stay unused: 0, 1 or 2 of them
      bool ok = legal;
      if (left != 0u && legal) {
        const uint64_t B1 = clear_full(B | (pr.shape << cell));
        const int b = __ffs((int)left) - 1;
        const uint64_t Ab = slot_anchors(t, hand, b, B1);
        if ((left & (left - 1u)) == 0u) {  // one piece left (wave-uniform)
          ok = Ab != 0ull;
        } else {  // two pieces left: some order, some anchor of its first piece
          const int c = 31 - __clz((int)left);
          const uint64_t Ac = slot_anchors(t, hand, c, B1);
          // Ab != 0 / Ac != 0 implies a valid id, so the clamped rows below are the pieces' own
          const uint32_t idb = hand_id(hand, b), idc = hand_id(hand, c);
          const uint64_t sb = t.row[idb < (uint32_t)kPieces ? idb : 0u].shape;
          const uint64_t sc = t.row[idc < (uint32_t)kPieces ? idc : 0u].shape;
          uint64_t mb = Ab, mc = Ac;
          ok = false;
#pragma unroll 1
          for (int it = 0; it < 64 && !ok && (mb | mc) != 0ull; ++it) {
            const int x = (__ffsll((unsigned long long)mb) - 1) & 63;
            const int y = (__ffsll((unsigned long long)mc) - 1) & 63;
            const bool leaf_b = (mb != 0ull) & (slot_anchors(t, hand, c, clear_full(B1 | (sb << x))) != 0ull);
            const bool leaf_c = (mc != 0ull) & (slot_anchors(t, hand, b, clear_full(B1 | (sc << y))) != 0ull);
            ok = leaf_b | leaf_c;
            mb &= mb - 1ull;  // 0 stays 0
            mc &= mc - 1ull;
          }
        }
      }
      legal_w[p] = __ballot(legal);
      safe_w[p] = __ballot(ok);
    }
    const bool keep = mode == BB_SAFE_WORDS || (safe_w[0] | safe_w[1] | safe_w[2]) != 0ull;  // wave-uniform
    const uint64_t w0 = keep ? safe_w[0] : legal_w[0];
    const uint64_t w1 = keep ? safe_w[1] : legal_w[1];
    const uint64_t w2 = keep ? safe_w[2] : legal_w[2];
    if (cell < kHand) mask[i * kHand + cell] = cell == 0 ? w0 : (cell == 1 ? w1 : w2);
  }
}

// ---------------------------------------------------------------------------
// Dealt next-hand values (bbvec.h bb_refill_values): the chance node behind a refill.  For (board i, deal j) the
// dealer of engine.py:155-172 on Philox words, then plan_kernel's search of the dealt hand.
//
// One workgroup of four waves per (board, deal) pair; above the grid cap the workgroups stride over the pairs
// (i, j advance by the grid size without a 64-bit division).
//   deal    the four waves test four consecutive draws at once: round r, wave k takes draw t = 4r + k.  Everything
//           of a draw is wave-uniform -- counter, Philox words and ids in scalar registers, the piece rows scalar
//           loads from the by-value table.  The acceptance test is safe_mask_kernel's existence search with the
//           wave leaving at the first lane that succeeds (census_kernel's full pass): lane = anchor of the first
//           piece, trip k tries the k-th lowest anchor of either order of the other two, the three choices of a
//           first piece in turn.  The waves post (ids, accepted) in LDS, one barrier per round (two buffers), and
//           the lowest accepted draw of the round wins; every wave reads the same four words, so all leave the
//           loop together.  At most 25 rounds; an open board ends in the first.
//   search  plan_kernel's body on the position (board, dealt hand, combo): plan_ply1 / plan_compact /
//           plan_record_turn<false> / plan_wave_join.  The key is carried and dropped at the end: it costs two
//           registers a lane, and the body stays the one the plan kernels use.
// Trip bounds: 25 rounds, 3 first pieces, 64 pair trips, <= 192 records, 3 slots, 64 mask bits.  No atomics, no
// inline assembly, nothing between workgroups.
// ---------------------------------------------------------------------------
constexpr int64_t kRefillMaxGrid = 1 << 14;  // more (board, deal) pairs than this: the workgroups stride over them
constexpr int kRefillRounds = kMaxAttempts / kPlanWaves;
static_assert(kRefillRounds * kPlanWaves == kMaxAttempts, "a round is one draw per wave");
constexpr uint32_t kRefillAccepted = 1u << 31;  // above the 18 id bits of a posted hand

struct RefillCols {
  const uint64_t* board;
  const int32_t* combo;    // NULL: 0
  const uint64_t* stream;  // NULL: i
};

// Can the whole hand (ids < kPieces, nothing used) be placed on B in some order?  Wave-uniform answer.
__device__ __forceinline__ bool hand_fits(const LookTable& t, uint64_t B, uint32_t hand, int cell) {
  bool found = false;
#pragma unroll 1
  for (int p = 0; p < kHand && !found; ++p) {
    const PieceRow& pa = t.row[hand_id(hand, p)];
    const PieceRow& pb = t.row[hand_id(hand, p == 0 ? 1 : 0)];
    const PieceRow& pc = t.row[hand_id(hand, p == 2 ? 1 : 2)];
    const bool legal = (anchors_of(pa, B) >> cell) & 1ull;
    const uint64_t B1 = clear_full(B | (pa.shape << cell));
    uint64_t mb = legal ? anchors_of(pb, B1) : 0ull;
    uint64_t mc = legal ? anchors_of(pc, B1) : 0ull;
#pragma unroll 1
    for (int it = 0; it < 64; ++it) {
      if (__ballot((mb | mc) != 0ull) == 0ull) break;  // every lane has run out of anchors
      const int y = (__ffsll((unsigned long long)mb) - 1) & 63;
      const int z = (__ffsll((unsigned long long)mc) - 1) & 63;
      const bool leaf_b = (mb != 0ull) & (anchors_of(pc, clear_full(B1 | (pb.shape << y))) != 0ull);
      const bool leaf_c = (mc != 0ull) & (anchors_of(pb, clear_full(B1 | (pc.shape << z))) != 0ull);
      mb &= mb - 1ull;  // 0 stays 0
      mc &= mc - 1ull;
      if (__ballot(leaf_b | leaf_c) != 0ull) {
        found = true;
        break;
      }
    }
  }
  return found;
}

__global__ void __launch_bounds__(kPlanBlock)
refill_values_kernel(LookTable t, RefillCols cols, int n, int m, bb_greedy_weights w, int depth, uint64_t seed,
                     bb_refill_values_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_deal[2][kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  const uint32_t um = (uint32_t)m;                                   // 1..1024
  const uint32_t gi = gridDim.x / um, gj = gridDim.x - gi * um;      // the stride in (i, j)
  int64_t i = (int64_t)(blockIdx.x / um);
  uint32_t j = blockIdx.x - (uint32_t)i * um;
  while (i < (int64_t)n) {
    const uint64_t B = uniform64(cols.board[i]);
    const int combo = (int)uniform32(cols.combo ? (uint32_t)cols.combo[i] : 0u);
    const uint64_t idx = cols.stream ? uniform64(cols.stream[i]) : (uint64_t)i;

    // ---- the deal
    uint32_t ids = 0u;
    int attempts = -kMaxAttempts;
#pragma unroll 1
    for (int r = 0; r < kRefillRounds; ++r) {
      uint32_t wd[4];
      philox_words(seed, idx, ((uint64_t)j << 7) | (uint64_t)(r * kPlanWaves + wave), wd);
      const uint32_t a = uniform32((uint32_t)(((uint64_t)wd[0] * (uint32_t)kPieces) >> 32));
      const uint32_t b = uniform32((uint32_t)(((uint64_t)wd[1] * (uint32_t)kPieces) >> 32));
      const uint32_t c = uniform32((uint32_t)(((uint64_t)wd[2] * (uint32_t)kPieces) >> 32));
      const uint32_t h = hand_pack(a, b, c, 0u, false, false);
      const bool ok = hand_fits(t, B, h, cell);
      if (cell == 0) s_deal[r & 1][wave] = h | (ok ? kRefillAccepted : 0u);
      __syncthreads();  // the other buffer is rewritten only after the next round's barrier: every wave has read this one
      const uint32_t d0 = uniform32(s_deal[r & 1][0]), d1 = uniform32(s_deal[r & 1][1]);
      const uint32_t d2 = uniform32(s_deal[r & 1][2]), d3 = uniform32(s_deal[r & 1][3]);
      const int k = (d0 & kRefillAccepted) ? 0 : (d1 & kRefillAccepted) ? 1 : (d2 & kRefillAccepted) ? 2 : 3;
      const uint32_t dk = k == 0 ? d0 : (k == 1 ? d1 : (k == 2 ? d2 : d3));
      ids = dk & kHandIds;  // the round's first accepted draw, else its last one (the 100th in the last round)
      if (dk & kRefillAccepted) {
        attempts = r * kPlanWaves + k + 1;
        break;  // the same four words in every wave: the workgroup leaves together
      }
    }

    // ---- the search of the dealt hand (plan_kernel's body)
    const Position P{B, ids, combo};
    int64_t best = INT64_MIN;  // below every legal value (see greedy_kernel)
    uint32_t best_key = kPlanNoKey;
    int leaves = 0;
    bool unused = false;
    const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
    if (ply1.closed) {
      best = move_terms(w, ply1.a) + state_terms(w, ply1.a);
      best_key = ((uint32_t)(wave * 64 + cell) << 16) | 0xFFFFu;
    }
    const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);
    for (int r = wave; r < total; r += kPlanWaves)
      plan_record_turn<false>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, unused);
    plan_wave_join(best, best_key, leaves);
    if (cell == 0) s_v[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < kPlanWaves; ++k) best = s_v[k] > best ? s_v[k] : best;
      const int64_t o = i * (int64_t)m + (int64_t)j;
      if (out.hand) out.hand[o] = ids;
      if (out.value) out.value[o] = best == INT64_MIN ? (int64_t)w.dead : best;  // no legal first move
      if (out.attempts) out.attempts[o] = attempts;
    }
    // no barrier here: the next pair's first LDS writes are s_deal, s_cnt and s_rec; s_v is rewritten only after
    // barriers that thread 0 has to reach first

    j += gj;
    i += (int64_t)gi;
    if (j >= um) {
      j -= um;
      ++i;
    }
  }
}

// refill_values_kernel's two halves restated for refill_values_ext_kernel; the parent keeps its own text for the
// reason given at plan_values_search (49 -> 52 VGPRs when it called these).
// The deal of pair (board B, stream idx, deal j): the hand's ids and the attempts (negative: nothing accepted).  The
// one barrier per round is met by the whole workgroup.  No weights are read, so this half is no template.
__device__ __forceinline__ void refill_deal(const LookTable& t, uint64_t B, uint64_t seed, uint64_t idx, uint32_t j,
                                            int wave, int cell, uint32_t (*s_deal)[kPlanWaves], uint32_t& ids,
                                            int& attempts) {
  ids = 0u;
  attempts = -kMaxAttempts;
#pragma unroll 1
  for (int r = 0; r < kRefillRounds; ++r) {
    uint32_t wd[4];
    philox_words(seed, idx, ((uint64_t)j << 7) | (uint64_t)(r * kPlanWaves + wave), wd);
    const uint32_t a = uniform32((uint32_t)(((uint64_t)wd[0] * (uint32_t)kPieces) >> 32));
    const uint32_t b = uniform32((uint32_t)(((uint64_t)wd[1] * (uint32_t)kPieces) >> 32));
    const uint32_t c = uniform32((uint32_t)(((uint64_t)wd[2] * (uint32_t)kPieces) >> 32));
    const uint32_t h = hand_pack(a, b, c, 0u, false, false);
    const bool ok = hand_fits(t, B, h, cell);
    if (cell == 0) s_deal[r & 1][wave] = h | (ok ? kRefillAccepted : 0u);
    __syncthreads();  // the other buffer is rewritten only after the next round's barrier: every wave has read this one
    const uint32_t d0 = uniform32(s_deal[r & 1][0]), d1 = uniform32(s_deal[r & 1][1]);
    const uint32_t d2 = uniform32(s_deal[r & 1][2]), d3 = uniform32(s_deal[r & 1][3]);
    const int k = (d0 & kRefillAccepted) ? 0 : (d1 & kRefillAccepted) ? 1 : (d2 & kRefillAccepted) ? 2 : 3;
    const uint32_t dk = k == 0 ? d0 : (k == 1 ? d1 : (k == 2 ? d2 : d3));
    ids = dk & kHandIds;  // the round's first accepted draw, else its last one (the 100th in the last round)
    if (dk & kRefillAccepted) {
      attempts = r * kPlanWaves + k + 1;
      break;  // the same four words in every wave: the workgroup leaves together
    }
  }
}

// The search of the dealt hand under either weight type (refill_values_ext_kernel's two sides): plan_kernel's body up
// to the wave join, the value alone kept.  Both barriers of plan_compact are inside.
template <class W>
__device__ __forceinline__ int64_t refill_search(const LookTable& t, const Position& P, const W& w, int depth, int wave,
                                                 int cell, PlanRecord* s_rec, int* s_cnt) {
  int64_t best = INT64_MIN;  // below every legal value (see greedy_kernel)
  uint32_t best_key = kPlanNoKey;
  int leaves = 0;
  bool unused = false;
  const Ply1 ply1 = plan_ply1(t, P, depth, wave, cell);
  if (ply1.closed) {
    best = move_terms(w, ply1.a) + state_terms(w, ply1.a);
    best_key = ((uint32_t)(wave * 64 + cell) << 16) | 0xFFFFu;
  }
  const int total = plan_compact(s_rec, s_cnt, w, ply1, wave, cell);
  for (int r = wave; r < total; r += kPlanWaves)
    plan_record_turn<false>(t, s_rec[r], P.hand, w, depth, cell, best, best_key, leaves, unused);
  plan_wave_join(best, best_key, leaves);
  return best;
}

// refill_values_kernel under rows of bb_eval_weights (bbvec.h bb_refill_values_ext): every deal of board i is searched
// under rows[i * w_stride], w_stride 0 or 1, read inside the pair loop into scalar registers.  The deal reads no
// weights and is the parent's.  The search has plan_ext_kernel's two sides; the branch is the workgroup's (every wave
// read the same row) and both sides meet the two barriers of plan_compact.  A hand without a legal first move gets
// w.base.dead alone: there is no afterstate whose board the shape terms could read.
__global__ void __launch_bounds__(kPlanBlock)
refill_values_ext_kernel(LookTable t, RefillCols cols, int n, int m, const bb_eval_weights* __restrict__ rows,
                         int64_t w_stride, int depth, uint64_t seed, bb_refill_values_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_deal[2][kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  const uint32_t um = (uint32_t)m;                                   // 1..1024
  const uint32_t gi = gridDim.x / um, gj = gridDim.x - gi * um;      // the stride in (i, j)
  int64_t i = (int64_t)(blockIdx.x / um);
  uint32_t j = blockIdx.x - (uint32_t)i * um;
  while (i < (int64_t)n) {
    const uint64_t B = uniform64(cols.board[i]);
    const int combo = (int)uniform32(cols.combo ? (uint32_t)cols.combo[i] : 0u);
    const uint64_t idx = cols.stream ? uniform64(cols.stream[i]) : (uint64_t)i;
    const bb_eval_weights w = load_eval_weights(rows, i * w_stride);  // every deal of board i: board i's row
    const bool shaped = (w.perimeter | w.room3 | w.room5 | w.fits) != 0;  // scalar: one answer for the workgroup

    // ---- the deal
    uint32_t ids;
    int attempts;
    refill_deal(t, B, seed, idx, j, wave, cell, s_deal, ids, attempts);

    // ---- the search of the dealt hand (plan_kernel's body)
    const Position P{B, ids, combo};
    int64_t best;
    if (shaped)
      best = refill_search(t, P, w, depth, wave, cell, s_rec, s_cnt);
    else
      best = refill_search(t, P, w.base, depth, wave, cell, s_rec, s_cnt);
    if (cell == 0) s_v[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 1; k < kPlanWaves; ++k) best = s_v[k] > best ? s_v[k] : best;
      const int64_t o = i * (int64_t)m + (int64_t)j;
      if (out.hand) out.hand[o] = ids;
      if (out.value) out.value[o] = best == INT64_MIN ? (int64_t)w.base.dead : best;  // no legal first move
      if (out.attempts) out.attempts[o] = attempts;
    }
    // no barrier here: the next pair's first LDS writes are s_deal, s_cnt and s_rec; s_v is rewritten only after
    // barriers that thread 0 has to reach first

    j += gj;
    i += (int64_t)gi;
    if (j >= um) {
      j -= um;
      ++i;
    }
  }
}

// ---------------------------------------------------------------------------
// Dealt playouts (bbvec.h bb_playout_values): refill_values_ext_kernel's pair, carried on for `hands` hands.  For
// (board i, playout j): deal under key seed + h, search the dealt hand, play the plan found, deal again on the board
// reached -- the plan agent under a counter-based dealer, the board held by the workgroup from the first deal to the
// last ply.
//
// refill_values_ext_kernel's frame: one workgroup of four waves per (board, playout) pair, the same two-digit stride
// above kRefillMaxGrid, the row read per pair into scalar registers, the `shaped` branch the workgroup's.  Inside the
// pair loop, per hand:
//   deal    refill_deal as it stands, its key seed + h (unsigned: it wraps mod 2^64).
//   search  plan_search<W> on either side of the branch, plan_wave_join, and lane 0 of each wave posts its (value, key)
//           in s_v / s_key.
//   join    after one barrier EVERY lane reads the four slots and joins them under take_plan, so the whole workgroup
//           holds the same (value, key), told to be uniform: the plan is in scalar registers.
//   play    the up to three plies of the key with eval_action on workgroup-uniform arguments (every lane computes the
//           same afterstate; the piece rows are scalar loads).  The state reached goes back into scalar registers.
// "No legal first move", "the leaf is no refill" and "this was the last hand" are therefore one answer for the
// workgroup: all four waves leave the hand loop together, and every barrier inside refill_deal and plan_compact is met
// by all of them.  Thread 0 stores the nine outputs once per pair.
//
// LDS reuse.  s_v / s_key are written by the lanes 0 before the join barrier and read by every lane after it; nothing
// else reads them.  Their next writes come
//   across hands   after the next hand's refill_deal (its first round always runs and has a barrier) and the two
//                  barriers of plan_compact;
//   across pairs   the same: the next pair opens with refill_deal;
//   on the early exit with no legal first move   the same again: the break leads to the stores and the next pair's
//                  refill_deal, or out of the kernel.
// A wave reaches any of those barriers only after its own reads of the slots, which precede them in program order, so
// the first barrier of the next refill_deal separates every read from the next write.  s_deal, s_cnt and s_rec are
// used as refill_values_ext_kernel uses them; between a hand's last read of them and the next hand's first write lies
// at least the join barrier.
// Trip bounds: `hands` <= 256 times (25 rounds, 3 first pieces, 64 pair trips; <= 192 records, 3 slots, 64 mask bits;
// 3 plies).  No atomics, no inline assembly, nothing between workgroups.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kPlanBlock)
playout_values_kernel(LookTable t, RefillCols cols, int n, int m, const bb_eval_weights* __restrict__ rows,
                      int64_t w_stride, int depth, int hands, uint64_t seed, bb_playout_out out) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_key[kPlanWaves];
  __shared__ uint32_t s_deal[2][kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  const uint32_t um = (uint32_t)m;                                   // 1..1024
  const uint32_t gi = gridDim.x / um, gj = gridDim.x - gi * um;      // the stride in (i, j)
  int64_t i = (int64_t)(blockIdx.x / um);
  uint32_t j = blockIdx.x - (uint32_t)i * um;
  while (i < (int64_t)n) {
    uint64_t B = uniform64(cols.board[i]);
    int combo = (int)uniform32(cols.combo ? (uint32_t)cols.combo[i] : 0u);
    const uint64_t idx = cols.stream ? uniform64(cols.stream[i]) : (uint64_t)i;
    const bb_eval_weights w = load_eval_weights(rows, i * w_stride);  // every playout of board i: board i's row
    const bool shaped = (w.perimeter | w.room3 | w.room5 | w.fits) != 0;  // scalar: one answer for the workgroup

    int64_t moved = 0, score = 0, value = 0;
    int lines = 0, plies = 0, searched = 0;
    uint32_t ids = 0u, status = 0u;
#pragma unroll 1
    for (int h = 0; h < hands; ++h) {
      // ---- the deal
      int attempts;
      refill_deal(t, B, seed + (uint64_t)h, idx, j, wave, cell, s_deal, ids, attempts);

      // ---- the search of the dealt hand (plan_ext_kernel's two sides)
      const Position P{B, ids, combo};
      int64_t best = INT64_MIN;  // below every legal value (see greedy_kernel)
      uint32_t best_key = kPlanNoKey;
      int leaves = 0;
      if (shaped)
        plan_search(t, P, w, depth, wave, cell, s_rec, s_cnt, best, best_key, leaves);
      else
        plan_search(t, P, w.base, depth, wave, cell, s_rec, s_cnt, best, best_key, leaves);
      plan_wave_join(best, best_key, leaves);
      if (cell == 0) {
        s_v[wave] = best;
        s_key[wave] = best_key;
      }
      __syncthreads();

      // ---- the join, by every lane: one (value, key) for the workgroup
      best = s_v[0];
      best_key = s_key[0];
#pragma unroll
      for (int k = 1; k < kPlanWaves; ++k) take_plan(best, best_key, s_v[k], s_key[k]);
      best = (int64_t)uniform64((uint64_t)best);
      best_key = uniform32(best_key);
      searched = h + 1;
      if (best_key == kPlanNoKey) {  // no legal first move: nothing is played
        value = moved + (int64_t)w.base.dead;
        status = 0u;
        break;
      }
      value = moved + best;

      // ---- the plan played (play_plan_kernel's plies; every entry is legal: the search placed it)
      uint32_t hand = ids;
      int64_t m_h = 0;
#pragma unroll 1
      for (int k = 0; k < kHand; ++k) {
        const uint32_t act = (best_key >> (16 - 8 * k)) & 0xFFu;
        if (act == 0xFFu) break;  // a ply not played
        const int p = (int)(act >> 6);
        const After a = eval_action(t, B, hand, combo, p, (int)(act & 63u));
        B = uniform64(a.board);
        hand = hand_use(hand, p);
        combo = (int)uniform32((uint32_t)a.combo1);
        const int l = (int)uniform32((uint32_t)a.lines);
        const int64_t g = (int64_t)uniform64((uint64_t)(int64_t)a.gained);
        lines += l;
        score += g;
        ++plies;
        m_h += (int64_t)w.base.lines * l + (int64_t)w.base.score * g;
        status = uniform32((uint32_t)(k + 1) | (a.dead ? BB_PLAY_DEAD : 0u) | (a.refill ? BB_PLAY_REFILL : 0u));
      }
      if (!(status & BB_PLAY_REFILL)) break;  // a dead leaf, or a plan cut short by depth < 3
      moved += m_h;  // used by the next hand alone: the last hand's value is already in place
    }

    if (threadIdx.x == 0) {
      const int64_t o = i * (int64_t)m + (int64_t)j;
      if (out.value) out.value[o] = value;
      if (out.score) out.score[o] = score;
      if (out.lines) out.lines[o] = lines;
      if (out.plies) out.plies[o] = plies;
      if (out.hands) out.hands[o] = searched;
      if (out.status) out.status[o] = (int32_t)status;
      if (out.board) out.board[o] = B;
      if (out.combo) out.combo[o] = combo;
      if (out.hand) out.hand[o] = ids;
    }

    j += gj;
    i += (int64_t)gi;
    if (j >= um) {
      j -= um;
      ++i;
    }
  }
}

// ---------------------------------------------------------------------------
// A plan played to its leaf (bbvec.h bb_play_plan_pos): one lane per position, up to three one-ply moves
// (eval_action, the move of every kernel above).  The pieces differ from lane to lane, so the table is copied into
// LDS once per workgroup, as census_kernel does.  Trip bound: 3 plies.  No atomics, no inline assembly.
// ---------------------------------------------------------------------------
constexpr int kPlayBlock = 256;
constexpr int64_t kPlayMaxGrid = 1 << 15;
constexpr int kRowWords = (int)(sizeof(PieceRow) / sizeof(uint64_t));
static_assert(sizeof(PieceRow) % sizeof(uint64_t) == 0, "the table is copied to LDS as 64-bit words");

__global__ void __launch_bounds__(kPlayBlock)
play_plan_kernel(LookTable t, LookPos pos, int n, const int32_t* __restrict__ plan, bb_play_plan_out out) {
  __shared__ LookTable s_t;
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&t);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&s_t);
    for (int k = (int)threadIdx.x; k < kPieces * kRowWords; k += kPlayBlock) dst[k] = src[k];
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kPlayBlock;
  for (int64_t i = (int64_t)blockIdx.x * kPlayBlock + threadIdx.x; i < (int64_t)n; i += stride) {
    uint64_t B = pos.board[i];
    uint32_t hand = pos.hand[i];
    int combo = pos.combo ? pos.combo[i] : 0;
    int lines = 0;
    int64_t score = 0;
    uint32_t status = 0u;
    bool go = true;
#pragma unroll 1
    for (int k = 0; k < kHand; ++k) {
      const int act = plan[i * kHand + k];
      go = go && act >= 0;
      if (!go) continue;
      const int p = act >> 6;
      if (p >= kHand) {  // not an action
        status |= BB_PLAY_ILLEGAL;
        go = false;
        continue;
      }
      const After a = eval_action(s_t, B, hand, combo, p, act & 63);
      if (!a.legal) {
        status |= BB_PLAY_ILLEGAL;
        go = false;
        continue;
      }
      B = a.board;
      hand = hand_use(hand, p);
      combo = a.combo1;
      lines += a.lines;
      score += a.gained;
      status = (uint32_t)(k + 1) | (a.dead ? BB_PLAY_DEAD : 0u) | (a.refill ? BB_PLAY_REFILL : 0u);
    }
    if (out.board) out.board[i] = B;
    if (out.hand) out.hand[i] = hand;
    if (out.combo) out.combo[i] = combo;
    if (out.lines) out.lines[i] = lines;
    if (out.score) out.score[i] = score;
    if (out.status) out.status[i] = (int32_t)status;
  }
}

// ---------------------------------------------------------------------------
// The two-hand decision (bbvec.h bb_plan2_values): three kernels behind a plan_values_ext_kernel launch that wrote
// q [n][192] and rest [n][192] into the caller's workspace.  Everything between the launches lives in that workspace
// (Plan2Work below); nothing is read back by the host.
//
//   plan2_candidates_kernel  one wave (one workgroup of 64) per position.  The 192 q go into LDS; lane l ranks its
//       three actions l, l + 64, l + 128 by counting, 192 broadcast reads each:
//       rank(a) = #{b : q[b] > q[a] or (q[b] == q[a] and b < a)}, the place of a in a stable descending sort.  Every
//       legal action is above INT64_MIN, so the legal ones hold the ranks 0..L-1.  A lane whose action is legal with
//       rank < K plays (a, decoded rest[a]) with eval_action and writes slot `rank` of the position: cand, the leaf's
//       board and combo, its move terms under the root's row and play_plan_kernel's status word.  Slots L..K-1 get
//       cand = status = -1.  The slots differ by lane, so the piece table is copied to LDS once per workgroup, as
//       play_plan_kernel does.  Trip bounds: 192 compares, 3 actions, 3 plies.
//   plan2_deal_kernel  one workgroup of four waves per (position, candidate, deal) triple; above the grid cap the
//       workgroups stride over the triples, (i, k * deals + j) advancing by the grid size as two digits, without a
//       64-bit division.  A candidate that is absent or whose leaf is no refill gets value 0 from thread 0 and the
//       workgroup goes on before it meets a barrier (the status word is read at a uniform index: one answer for the
//       workgroup).  Otherwise refill_deal and refill_search<W> as refill_values_ext_kernel calls them, on the leaf's
//       board and combo under the root's row and stream id.  Trip bounds: those of refill_values_ext_kernel.
//   plan2_pick_kernel  one wave (one workgroup of 64) per position.  Lane l takes the candidates l, l + 64, l + 128:
//       Q2 = deals * moved + sum of the dealt values for a refill leaf, deals * q[a] for any other, staged in an LDS
//       row of 192 that starts as INT64_MIN; the lanes' best (Q2, action) are joined by shuffles under take_better
//       (the larger value, then the lower action -- not the lower rank) and the row is stored, 64 consecutive
//       elements per store.  Trip bounds: 3 candidates a lane, `deals` values each.
// No atomics, no inline assembly, nothing between workgroups.
// ---------------------------------------------------------------------------
constexpr int kPlan2Block = 64;                  // candidates and pick: one wave is one workgroup
constexpr int64_t kPlan2DealMaxGrid = 1 << 14;   // more triples than this: the workgroups stride over them

struct Plan2Work {   // the workspace as launch_plan2_values carves it (bb_look_rules.h Plan2Layout holds the offsets)
  int64_t* q;        // [n][192]
  uint64_t* board;   // [n][K] the leaf's board
  int64_t* moved;    // [n][K] w.base.lines * lines + w.base.score * score over the plies played
  int64_t* value;    // [n][K][deals] (the caller's own array when it asked for one)
  int32_t* rest;     // [n][192]
  int32_t* combo;    // [n][K] the leaf's combo
  int32_t* cand;     // [n][K] (the caller's own array when it asked for one)
  int32_t* status;   // [n][K] (the caller's own array when it asked for one)
};

__global__ void __launch_bounds__(kPlan2Block)
plan2_candidates_kernel(LookTable t, LookPos pos, int n, const bb_eval_weights* __restrict__ rows, int64_t w_stride,
                        int K, Plan2Work wk) {
  __shared__ LookTable s_t;
  __shared__ int64_t s_q[BB_ACTIONS];
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&t);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&s_t);
    for (int k = (int)threadIdx.x; k < kPieces * kRowWords; k += kPlan2Block) dst[k] = src[k];
  }
  const int lane = (int)threadIdx.x;
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    __syncthreads();  // the table is in place; the last position's q have been read by every lane
    int64_t qa[kHand];
#pragma unroll
    for (int s = 0; s < kHand; ++s) {
      qa[s] = wk.q[i * BB_ACTIONS + (int64_t)(s * 64 + lane)];
      s_q[s * 64 + lane] = qa[s];
    }
    __syncthreads();
    int rank[kHand] = {0, 0, 0};
#pragma unroll 4
    for (int b = 0; b < BB_ACTIONS; ++b) {
      const int64_t qb = s_q[b];  // one address for the wave: a broadcast read
#pragma unroll
      for (int s = 0; s < kHand; ++s) rank[s] += (int)(qb > qa[s] || (qb == qa[s] && b < s * 64 + lane));
    }
    int legal = 0;  // L: the legal actions hold the ranks 0..L-1
#pragma unroll
    for (int s = 0; s < kHand; ++s) legal += __popcll(__ballot(qa[s] != INT64_MIN));
    const int32_t lines_w = rows[i * w_stride].base.lines, score_w = rows[i * w_stride].base.score;
#pragma unroll 1
    for (int s = 0; s < kHand; ++s) {
      // selects, not qa[s] / rank[s]: an array indexed by a loop counter that is not unrolled would live in scratch
      const int64_t qs = s == 0 ? qa[0] : (s == 1 ? qa[1] : qa[2]);
      const int slot = s == 0 ? rank[0] : (s == 1 ? rank[1] : rank[2]);
      if (qs == INT64_MIN || slot >= K) continue;
      const int a1 = s * 64 + lane;
      const int32_t rest = wk.rest[i * BB_ACTIONS + (int64_t)a1];
      const int r2 = rest & 0xFF, r3 = (rest >> 8) & 0xFF;
      const int a2 = r2 == 0xFF ? -1 : r2, a3 = r3 == 0xFF ? -1 : r3;
      uint64_t B = pos.board[i];
      uint32_t hand = pos.hand[i];
      int combo = pos.combo ? pos.combo[i] : 0;
      int64_t moved = 0;
      uint32_t status = 0u;
      bool go = true;
#pragma unroll 1
      for (int k = 0; k < kHand; ++k) {  // play_plan_kernel's plies
        const int act = k == 0 ? a1 : (k == 1 ? a2 : a3);
        go = go && act >= 0;
        if (!go) continue;
        const int p = act >> 6;
        if (p >= kHand) {  // not an action
          status |= BB_PLAY_ILLEGAL;
          go = false;
          continue;
        }
        const After a = eval_action(s_t, B, hand, combo, p, act & 63);
        if (!a.legal) {
          status |= BB_PLAY_ILLEGAL;
          go = false;
          continue;
        }
        B = a.board;
        hand = hand_use(hand, p);
        combo = a.combo1;
        moved += (int64_t)lines_w * a.lines + (int64_t)score_w * a.gained;
        status = (uint32_t)(k + 1) | (a.dead ? BB_PLAY_DEAD : 0u) | (a.refill ? BB_PLAY_REFILL : 0u);
      }
      const int64_t o = i * (int64_t)K + (int64_t)slot;  // slot < K
      wk.cand[o] = a1;
      wk.board[o] = B;
      wk.combo[o] = combo;
      wk.moved[o] = moved;
      wk.status[o] = (int32_t)status;
    }
    for (int r = legal + lane; r < K; r += kPlan2Block) {  // the absent candidates
      wk.cand[i * (int64_t)K + (int64_t)r] = -1;
      wk.status[i * (int64_t)K + (int64_t)r] = -1;
    }
  }
}

__global__ void __launch_bounds__(kPlanBlock)
plan2_deal_kernel(LookTable t, const uint64_t* __restrict__ stream_id, int n, int K, int m,
                  const bb_eval_weights* __restrict__ rows, int64_t w_stride, int depth, uint64_t seed,
                  const int32_t* __restrict__ leaf_status, const uint64_t* __restrict__ leaf_board,
                  const int32_t* __restrict__ leaf_combo, int64_t* __restrict__ value) {
  __shared__ PlanRecord s_rec[kPlanRecords];
  __shared__ int s_cnt[kHand];
  __shared__ int64_t s_v[kPlanWaves];
  __shared__ uint32_t s_deal[2][kPlanWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cell = (int)(threadIdx.x & 63u);
  // two digits as in refill_values_ext_kernel: the root i, and kj = k * m + j of radix K * m <= 196,608; the grid size
  // is added digit by digit, and k, j come back from kj by one 32-bit division a triple
  const uint32_t um = (uint32_t)m, ukm = (uint32_t)K * um;
  const uint32_t gi = gridDim.x / ukm, gkj = gridDim.x - gi * ukm;   // the stride in (i, kj)
  int64_t i = (int64_t)(blockIdx.x / ukm);
  uint32_t kj = blockIdx.x - (uint32_t)i * ukm;
  while (i < (int64_t)n) {
    const uint32_t k = kj / um, j = kj - k * um;
    const int64_t c = i * (int64_t)K + (int64_t)k;
    const int64_t o = i * (int64_t)ukm + (int64_t)kj;
    const int32_t status = (int32_t)uniform32((uint32_t)leaf_status[c]);
    if (status < 0 || !((uint32_t)status & BB_PLAY_REFILL)) {  // the workgroup's answer: no barrier is met on this side
      if (threadIdx.x == 0) value[o] = 0;
    } else {
    const uint64_t B = uniform64(leaf_board[c]);
    const int combo = (int)uniform32((uint32_t)leaf_combo[c]);
    const uint64_t idx = stream_id ? uniform64(stream_id[i]) : (uint64_t)i;  // the root's: one stream for its candidates
    const bb_eval_weights w = load_eval_weights(rows, i * w_stride);       // the root's row
    const bool shaped = (w.perimeter | w.room3 | w.room5 | w.fits) != 0;     // scalar: one answer for the workgroup

    uint32_t ids;
    int attempts;
    refill_deal(t, B, seed, idx, j, wave, cell, s_deal, ids, attempts);
    const Position P{B, ids, combo};
    int64_t best;
    if (shaped)
      best = refill_search(t, P, w, depth, wave, cell, s_rec, s_cnt);
    else
      best = refill_search(t, P, w.base, depth, wave, cell, s_rec, s_cnt);
    if (cell == 0) s_v[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int v = 1; v < kPlanWaves; ++v) best = s_v[v] > best ? s_v[v] : best;
      value[o] = best == INT64_MIN ? (int64_t)w.base.dead : best;  // no legal first move
    }
    // no barrier here, as in refill_values_ext_kernel: a triple that is skipped touches no LDS at all
    }

    kj += gkj;
    i += (int64_t)gi;
    if (kj >= ukm) {
      kj -= ukm;
      ++i;
    }
  }
}

__global__ void __launch_bounds__(kPlan2Block)
plan2_pick_kernel(int n, int K, int m, Plan2Work wk, int32_t* __restrict__ action, int64_t* __restrict__ q2) {
  __shared__ int64_t s_q2[BB_ACTIONS];
  const int lane = (int)threadIdx.x;
  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
#pragma unroll
    for (int s = 0; s < kHand; ++s) s_q2[s * 64 + lane] = INT64_MIN;
    __syncthreads();
    int64_t v = INT64_MIN;  // below every Q2 (see greedy_kernel): a lane without a candidate never wins
    int act = BB_ACTIONS;
    for (int r = lane; r < K; r += kPlan2Block) {  // at most three candidates a lane
      const int64_t c = i * (int64_t)K + (int64_t)r;
      const int a = wk.cand[c];
      if (a < 0) continue;
      int64_t x;
      if ((uint32_t)wk.status[c] & BB_PLAY_REFILL) {
        x = (int64_t)m * wk.moved[c];
        for (int j = 0; j < m; ++j) x += wk.value[c * (int64_t)m + (int64_t)j];
      } else {
        x = (int64_t)m * wk.q[i * BB_ACTIONS + (int64_t)a];
      }
      s_q2[a] = x;  // the candidates of a position are distinct actions
      take_better(v, act, x, a);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int64_t v2 = __shfl_xor(v, d, 64);
      const int act2 = __shfl_xor(act, d, 64);
      take_better(v, act, v2, act2);
    }
    __syncthreads();
    if (action && lane == 0) action[i] = act == BB_ACTIONS ? 0 : act;
    if (q2) {
#pragma unroll
      for (int s = 0; s < kHand; ++s) q2[i * BB_ACTIONS + (int64_t)(s * 64 + lane)] = s_q2[s * 64 + lane];
    }
    __syncthreads();  // the row is rewritten by the workgroup's next position
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
inline dim3 plan_grid(int n) { return dim3((unsigned)((int64_t)n < kPlanMaxGrid ? (int64_t)n : kPlanMaxGrid)); }

}  // namespace

hipError_t launch_afterstates(const uint64_t* board, const uint32_t* hand, const int32_t* combo, const uint16_t* prev,
                              int n, const bb_reward_cfg& cfg, const bb_afterstate_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, prev};
  hipLaunchKernelGGL(afterstates_kernel, look_grid(n), dim3(kLookBlock), 0, s, look_table(), pos, n, cfg,
                     cfg.center_bonus * 0.1, out);
  return hipGetLastError();
}

hipError_t launch_greedy(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                         const bb_greedy_weights& w, int32_t* action, int64_t* value, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  hipLaunchKernelGGL(greedy_kernel, look_grid(n), dim3(kLookBlock), 0, s, look_table(), pos, n, w, action, value);
  return hipGetLastError();
}

hipError_t launch_greedy_each(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                              const bb_greedy_weights* rows, int32_t* action, int64_t* value, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  hipLaunchKernelGGL(greedy_each_kernel, look_grid(n), dim3(kLookBlock), 0, s, look_table(), pos, n, rows, action,
                     value);
  return hipGetLastError();
}

hipError_t launch_plan(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                       const bb_greedy_weights& w, int depth, const bb_plan_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  hipLaunchKernelGGL(plan_kernel, plan_grid(n), dim3(kPlanBlock), 0, s, look_table(), pos, n, w, depth, out);
  return hipGetLastError();
}

hipError_t launch_plan_each(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                            const bb_greedy_weights* rows, int depth, const bb_plan_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  hipLaunchKernelGGL(plan_each_kernel, plan_grid(n), dim3(kPlanBlock), 0, s, look_table(), pos, n, rows, depth, out);
  return hipGetLastError();
}

hipError_t launch_plan_ext(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                           const bb_eval_weights* rows, int64_t w_stride, int depth, const bb_plan_out& out,
                           hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  hipLaunchKernelGGL(plan_ext_kernel, plan_grid(n), dim3(kPlanBlock), 0, s, look_table(), pos, n, rows, w_stride, depth,
                     out);
  return hipGetLastError();
}

hipError_t launch_board_terms(const uint64_t* board, int n, int32_t* terms, hipStream_t s) {
  const int64_t blocks = ((int64_t)n + kTermsBlock - 1) / kTermsBlock;
  const dim3 grid((unsigned)(blocks < kTermsMaxGrid ? blocks : kTermsMaxGrid));
  hipLaunchKernelGGL(board_terms_kernel, grid, dim3(kTermsBlock), 0, s, board, n, terms);
  return hipGetLastError();
}

hipError_t launch_plan_values(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                              const bb_greedy_weights& w, int depth, const bb_plan_values_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  // the safe set of depth 3 is that of depth 2 (bbvec.h): asked for alone, the third ply is not searched
  if (depth == 3 && !out.q && !out.rest && !out.leaves) depth = 2;
  hipLaunchKernelGGL(plan_values_kernel, plan_grid(n), dim3(kPlanBlock), 0, s, look_table(), pos, n, w, depth, out);
  return hipGetLastError();
}

hipError_t launch_plan_values_ext(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                                  const bb_eval_weights* rows, int64_t w_stride, int depth,
                                  const bb_plan_values_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  if (depth == 3 && !out.q && !out.rest && !out.leaves) depth = 2;  // as launch_plan_values
  hipLaunchKernelGGL(plan_values_ext_kernel, plan_grid(n), dim3(kPlanBlock), 0, s, look_table(), pos, n, rows, w_stride,
                     depth, out);
  return hipGetLastError();
}

hipError_t launch_safe_mask(const uint64_t* board, const uint32_t* hand, int n, int mode, uint64_t* mask,
                            hipStream_t s) {
  const LookPos pos{board, hand, nullptr, nullptr};
  const int64_t blocks = ((int64_t)n + kSafeWaves - 1) / kSafeWaves;
  const dim3 grid((unsigned)(blocks < kSafeMaxGrid ? blocks : kSafeMaxGrid));
  hipLaunchKernelGGL(safe_mask_kernel, grid, dim3(kSafeBlock), 0, s, look_table(), pos, n, mode, mask);
  return hipGetLastError();
}

hipError_t launch_refill_values(const uint64_t* board, const int32_t* combo, const uint64_t* stream_id, int n,
                                const bb_greedy_weights& w, int depth, int deals, uint64_t seed,
                                const bb_refill_values_out& out, hipStream_t s) {
  const RefillCols cols{board, combo, stream_id};
  const int64_t pairs = (int64_t)n * deals;
  const dim3 grid((unsigned)(pairs < kRefillMaxGrid ? pairs : kRefillMaxGrid));
  hipLaunchKernelGGL(refill_values_kernel, grid, dim3(kPlanBlock), 0, s, look_table(), cols, n, deals, w, depth, seed,
                     out);
  return hipGetLastError();
}

hipError_t launch_refill_values_ext(const uint64_t* board, const int32_t* combo, const uint64_t* stream_id, int n,
                                    const bb_eval_weights* rows, int64_t w_stride, int depth, int deals, uint64_t seed,
                                    const bb_refill_values_out& out, hipStream_t s) {
  const RefillCols cols{board, combo, stream_id};
  const int64_t pairs = (int64_t)n * deals;
  const dim3 grid((unsigned)(pairs < kRefillMaxGrid ? pairs : kRefillMaxGrid));
  hipLaunchKernelGGL(refill_values_ext_kernel, grid, dim3(kPlanBlock), 0, s, look_table(), cols, n, deals, rows,
                     w_stride, depth, seed, out);
  return hipGetLastError();
}

// bbvec.h bb_plan2_values: four launches on one stream, each reading what the one before wrote into the workspace
hipError_t launch_plan2_values(const uint64_t* board, const uint32_t* hand, const int32_t* combo,
                               const uint64_t* stream_id, int n, const bb_eval_weights* rows, int64_t w_stride,
                               int depth, int candidates, int deals, uint64_t seed, void* work,
                               const bb_plan2_out& out, hipStream_t s) {
  const bb_look_rules::Plan2Layout lay(n, candidates, deals);
  char* base = static_cast<char*>(work);
  Plan2Work wk;
  wk.q = reinterpret_cast<int64_t*>(base + lay.q);
  wk.board = reinterpret_cast<uint64_t*>(base + lay.board);
  wk.moved = reinterpret_cast<int64_t*>(base + lay.moved);
  wk.value = out.value ? out.value : reinterpret_cast<int64_t*>(base + lay.value);
  wk.rest = reinterpret_cast<int32_t*>(base + lay.rest);
  wk.combo = reinterpret_cast<int32_t*>(base + lay.combo);
  wk.cand = out.cand ? out.cand : reinterpret_cast<int32_t*>(base + lay.cand);
  wk.status = out.status ? out.status : reinterpret_cast<int32_t*>(base + lay.status);

  const LookPos pos{board, hand, combo, nullptr};
  const bb_plan_values_out pv{wk.q, wk.rest, nullptr, nullptr};
  hipLaunchKernelGGL(plan_values_ext_kernel, plan_grid(n), dim3(kPlanBlock), 0, s, look_table(), pos, n, rows, w_stride,
                     depth, pv);
  hipError_t st = hipGetLastError();
  if (st != hipSuccess) return st;
  const dim3 wave_grid((unsigned)((int64_t)n < kPlanMaxGrid ? (int64_t)n : kPlanMaxGrid));
  hipLaunchKernelGGL(plan2_candidates_kernel, wave_grid, dim3(kPlan2Block), 0, s, look_table(), pos, n, rows, w_stride,
                     candidates, wk);
  st = hipGetLastError();
  if (st != hipSuccess) return st;
  const int64_t triples = (int64_t)n * candidates * deals;
  const dim3 deal_grid((unsigned)(triples < kPlan2DealMaxGrid ? triples : kPlan2DealMaxGrid));
  hipLaunchKernelGGL(plan2_deal_kernel, deal_grid, dim3(kPlanBlock), 0, s, look_table(), stream_id, n, candidates,
                     deals, rows, w_stride, depth, seed, wk.status, wk.board, wk.combo, wk.value);
  st = hipGetLastError();
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(plan2_pick_kernel, wave_grid, dim3(kPlan2Block), 0, s, n, candidates, deals, wk, out.action,
                     out.q2);
  return hipGetLastError();
}

hipError_t launch_playout_values(const uint64_t* board, const int32_t* combo, const uint64_t* stream_id, int n,
                                 const bb_eval_weights* rows, int64_t w_stride, int depth, int playouts, int hands,
                                 uint64_t seed, const bb_playout_out& out, hipStream_t s) {
  const RefillCols cols{board, combo, stream_id};
  const int64_t pairs = (int64_t)n * playouts;
  const dim3 grid((unsigned)(pairs < kRefillMaxGrid ? pairs : kRefillMaxGrid));
  hipLaunchKernelGGL(playout_values_kernel, grid, dim3(kPlanBlock), 0, s, look_table(), cols, n, playouts, rows,
                     w_stride, depth, hands, seed, out);
  return hipGetLastError();
}

hipError_t launch_play_plan(const uint64_t* board, const uint32_t* hand, const int32_t* combo, int n,
                            const int32_t* plan, const bb_play_plan_out& out, hipStream_t s) {
  const LookPos pos{board, hand, combo, nullptr};
  const int64_t blocks = ((int64_t)n + kPlayBlock - 1) / kPlayBlock;
  const dim3 grid((unsigned)(blocks < kPlayMaxGrid ? blocks : kPlayMaxGrid));
  hipLaunchKernelGGL(play_plan_kernel, grid, dim3(kPlayBlock), 0, s, look_table(), pos, n, plan, out);
  return hipGetLastError();
}

}  // namespace bb
