// bb_census.hip -- the refill census (gfx950): bb_refill_census(_pos) of include/bbvec.h.
//
// For a board B, which of the 37^3 hands the dealer of engine.py:155-172 would accept, i.e. for which hands
// {a, b, c} the depth-first search of engine.py:174-224 (_can_place_all_pieces, with the line clears of
// engine.py:226-238 between the pieces) finds an order and anchors.  Integers only, nothing but the board is read,
// and no random number is drawn.  A file of its own, so that the kernels of bb_lookahead.hip compile to the
// instructions they had before this one existed.
//
// The algebra.  For a first piece a at anchor x, B1 = clear_full(B | a.shape << x).  The pair {b, c} fits B1 iff
// for one of the orders (b, c), (c, b) the first piece has an anchor y on B1 such that the second has an anchor
// on clear_full(B1 | first.shape << y).  S[a][b] bit c = "some anchor x of a on B leaves a B1 that {b, c} fits";
// S[a] is symmetric in (b, c).  Hand {a, b, c} is solvable iff S[a][b] has c, or S[b][a] has c, or S[c][a] has b
// (one term per choice of the first piece) -- so once one of the three is known, the other two need no search.
//
// Layout: one workgroup of sixteen waves per board; above the grid cap the workgroups stride.  A work item is
// (a, {b, c}) with b <= c: 37 * 703 = 26,011 items.  The 11 KB S table lives in LDS and takes the bits through LDS
// atomic ORs (a word S[a][b] is met by up to 37 items).
//   quick pass  lane = item (26 static trips of 1,024 threads).  The lane tries the kQuickX lowest anchors of a and
//               below each the kQuickY lowest anchors of either order (first leaves first, as pair_quick_bf and
//               safe_mask_kernel order them).  An open board settles every item at its first leaf.  An item that has
//               no anchor for a is settled too (nothing to find); any other failure sets the item's bit in the
//               pending bitmap.  The pieces differ from lane to lane, so the piece table (passed by value in the
//               kernel arguments, as the lookahead kernels take it) is copied into LDS once per workgroup.
//   full pass   wave = pending item, lane = anchor x of a, the pieces in scalar registers (read from the kernel
//               arguments at wave-uniform indices): all afterstates B1 of the item at once, and trip k tries the
//               k-th lowest anchor of either order in every lane -- safe_mask_kernel's search with the wave leaving
//               at the first lane that succeeds.  The waves take the bitmap words round-robin.  A hand already
//               known solvable through another first piece is skipped (a stale read of S costs a search, not a
//               wrong answer: the bits only ever get set, and each is an existence proof).
//   last pass   thread = word [a][b]: symmetrise over the three first pieces, store the word, count its bits.
// Trip bounds: 26 items per thread, kQuickX * kQuickY quick trips, 813 bitmap words of 32 bits, 64 pair trips, 37
// pieces.  No atomics on global memory, no inline assembly, no communication between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_env_internal.h"

namespace bb {

namespace {

constexpr int kCensusBlock = 1024;
constexpr int kCensusWaves = kCensusBlock / 64;
constexpr int kPairs = kPieces * (kPieces + 1) / 2;               // 703 multisets {b, c}
constexpr int kItems = kPieces * kPairs;                          // 26,011 (a, {b, c})
constexpr int kItemTrips = (kItems + kCensusBlock - 1) / kCensusBlock;
constexpr int kPendWords = (kItems + 31) / 32;                    // 813
constexpr int kWords = kPieces * kPieces;                         // 1,369 words [a][b] per board
constexpr int kRowWords = (int)(sizeof(PieceRow) / sizeof(uint64_t));
constexpr int kQuickX = 2, kQuickY = 2;      // the quick pass: anchors of a tried, pair trips below each
constexpr int64_t kCensusMaxGrid = 1 << 11;  // more boards than this: the workgroups stride over them

static_assert(sizeof(PieceRow) % sizeof(uint64_t) == 0, "the table is copied to LDS as 64-bit words");

struct CensusTable {
  PieceRow row[kPieces];
};

__device__ __forceinline__ int uniform_i(int x) { return __builtin_amdgcn_readfirstlane(x); }

// one pair trip on X: the lowest anchors of mb (pb then pc) and of mc (pc then pb), both leaves computed and
// or-ed so that the lanes of a wave stay on one path; the two masks lose their lowest bit (0 stays 0)
__device__ __forceinline__ bool pair_trip(const PieceRow& pb, const PieceRow& pc, uint64_t X, uint64_t& mb,
                                          uint64_t& mc) {
  const int y = (__ffsll((unsigned long long)mb) - 1) & 63;
  const int z = (__ffsll((unsigned long long)mc) - 1) & 63;
  const bool leaf_b = (mb != 0ull) & (anchors_of(pc, clear_full(X | (pb.shape << y))) != 0ull);
  const bool leaf_c = (mc != 0ull) & (anchors_of(pb, clear_full(X | (pc.shape << z))) != 0ull);
  mb &= mb - 1ull;
  mc &= mc - 1ull;
  return leaf_b | leaf_c;
}

__global__ void __launch_bounds__(kCensusBlock)
census_kernel(CensusTable t, const uint64_t* __restrict__ board, int n, bb_census_out out) {
  __shared__ PieceRow s_row[kPieces];
  __shared__ unsigned long long s_S[kWords];
  __shared__ uint32_t s_pend[kPendWords];
  __shared__ uint16_t s_pair[kPairs];  // b | c << 8 of pair r, b <= c
  __shared__ int s_cnt[kCensusWaves];
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = uniform_i(tid >> 6);

  // once per workgroup: the piece table and the pair list
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&t);
    uint64_t* dst = reinterpret_cast<uint64_t*>(s_row);
    for (int k = tid; k < kPieces * kRowWords; k += kCensusBlock) dst[k] = src[k];
    if (tid < kPieces) {
      const int b = tid, base = b * kPieces - (b * (b - 1)) / 2;  // pairs with a smaller first member
      for (int c = b; c < kPieces; ++c) s_pair[base + (c - b)] = (uint16_t)(b | (c << 8));  // < kPairs
    }
  }

  for (int64_t i = blockIdx.x; i < (int64_t)n; i += gridDim.x) {
    const uint64_t bw = board[i];
    const uint64_t B = ((uint64_t)(uint32_t)uniform_i((int)(uint32_t)(bw >> 32)) << 32) |
                       (uint32_t)uniform_i((int)(uint32_t)bw);
    for (int k = tid; k < kWords; k += kCensusBlock) s_S[k] = 0ull;
    for (int k = tid; k < kPendWords; k += kCensusBlock) s_pend[k] = 0u;
    __syncthreads();  // the table (first board), the cleared words and bitmap

    // ---- quick pass: lane = item
    for (int j = 0; j < kItemTrips; ++j) {
      const int w = j * kCensusBlock + tid;
      if (w >= kItems) continue;
      const int a = w / kPairs, r = w - a * kPairs;  // a < 37, r < 703
      const uint32_t bc = s_pair[r];
      const int b = (int)(bc & 0xFFu), c = (int)(bc >> 8);
      const PieceRow& pa = s_row[a];
      const PieceRow& pb = s_row[b];
      const PieceRow& pc = s_row[c];
      uint64_t ma = anchors_of(pa, B);
      bool ok = false, open = false;  // open: something was left untried
#pragma unroll 1
      for (int ix = 0; ix < kQuickX && !ok && ma != 0ull; ++ix) {
        const int x = __ffsll((unsigned long long)ma) - 1;
        ma &= ma - 1ull;
        const uint64_t B1 = clear_full(B | (pa.shape << x));
        uint64_t mb = anchors_of(pb, B1), mc = anchors_of(pc, B1);
#pragma unroll 1
        for (int it = 0; it < kQuickY && !ok && (mb | mc) != 0ull; ++it) ok = pair_trip(pb, pc, B1, mb, mc);
        open |= (mb | mc) != 0ull;
      }
      open |= ma != 0ull;
      if (ok) {
        atomicOr(&s_S[a * kPieces + b], 1ull << c);
        atomicOr(&s_S[a * kPieces + c], 1ull << b);
      } else if (open) {
        atomicOr(&s_pend[w >> 5], 1u << (w & 31));  // w >> 5 < kPendWords
      }
    }
    __syncthreads();

    // ---- full pass: wave = pending item, lane = anchor of a
    for (int pw = wave; pw < kPendWords; pw += kCensusWaves) {
      uint32_t bits = (uint32_t)uniform_i((int)s_pend[pw]);
      while (bits != 0u) {  // <= 32 trips
        const int w = pw * 32 + (__ffs((int)bits) - 1);  // < kItems: only such bits were set
        bits &= bits - 1u;
        const int a = w / kPairs, r = w - a * kPairs;
        const uint32_t bc = (uint32_t)uniform_i((int)s_pair[r]);
        const int b = (int)(bc & 0xFFu), c = (int)(bc >> 8);
        // the hand is already known solvable through some first piece: nothing to add (relaxed reads; see above)
        const unsigned long long known =
            ((__hip_atomic_load(&s_S[a * kPieces + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) |
              __hip_atomic_load(&s_S[b * kPieces + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >> c) |
            (__hip_atomic_load(&s_S[c * kPieces + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> b);
        if (uniform_i((int)(known & 1ull))) continue;
        const PieceRow& pa = t.row[a];
        const PieceRow& pb = t.row[b];
        const PieceRow& pc = t.row[c];
        const bool legal = (anchors_of(pa, B) >> lane) & 1ull;
        const uint64_t B1 = clear_full(B | (pa.shape << lane));
        uint64_t mb = legal ? anchors_of(pb, B1) : 0ull;
        uint64_t mc = legal ? anchors_of(pc, B1) : 0ull;
        bool found = false;
#pragma unroll 1
        for (int it = 0; it < 64; ++it) {
          if (__ballot((mb | mc) != 0ull) == 0ull) break;  // every lane has run out of anchors
          if (__ballot(pair_trip(pb, pc, B1, mb, mc)) != 0ull) {
            found = true;
            break;
          }
        }
        if (found && lane == 0) {
          atomicOr(&s_S[a * kPieces + b], 1ull << c);
          atomicOr(&s_S[a * kPieces + c], 1ull << b);
        }
      }
    }
    __syncthreads();

    // ---- last pass: symmetrise, store, count: thread = word [a][b]
    int cnt = 0;
    for (int k = tid; k < kWords; k += kCensusBlock) {
      const int a = k / kPieces, b = k - a * kPieces;
      uint64_t word = s_S[a * kPieces + b] | s_S[b * kPieces + a];
      for (int c = 0; c < kPieces; ++c) word |= ((s_S[c * kPieces + a] >> b) & 1ull) << c;
      if (out.solvable) out.solvable[i * kWords + k] = word;
      cnt += __popcll(word);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0 && out.count) {
      int total = 0;
#pragma unroll
      for (int k = 0; k < kCensusWaves; ++k) total += s_cnt[k];
      out.count[i] = total;
    }
    __syncthreads();  // s_S, s_pend and s_cnt are rewritten by the workgroup's next board
  }
}

const CensusTable& census_table() {
  static const CensusTable t = [] {
    CensusTable x;
    uint8_t dtab[kPieces * kPieces];
    build_piece_tables(x.row, dtab);
    return x;
  }();
  return t;
}

}  // namespace

hipError_t launch_refill_census(const uint64_t* board, int n, const bb_census_out& out, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)n < kCensusMaxGrid ? (int64_t)n : kCensusMaxGrid));
  hipLaunchKernelGGL(census_kernel, grid, dim3(kCensusBlock), 0, s, census_table(), board, n, out);
  return hipGetLastError();
}

}  // namespace bb
