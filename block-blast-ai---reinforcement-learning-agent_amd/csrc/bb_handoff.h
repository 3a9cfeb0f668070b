// bb_handoff.h -- the last-arriver hand-off between workgroups (gfx950), once: the primitives bb_optim.hip's
// split reductions and the three fused loss kernels use, and the loss kernels' block_sums_finish on top of them.
//
// Ordered by the HIP memory model rather than by hardware behaviour: partial sums stored with agent-scope atomic
// stores (written through, sc1), a workgroup barrier (every wave's stores issued before the count), then one lane
// counts the workgroup with an agent-scope release add (buffer_wbl2 sc1 + s_waitcnt vmcnt(0) before it: the
// partials of every wave that passed the barrier are published); the lane
// whose add returns the last count issues an agent-scope acquire fence (buffer_inv sc1) before its workgroup --
// after a barrier, or in the same wave -- loads the partials with agent-scope loads.  The other workgroups skip
// the acquire (acq_rel on every add: 1.510 against 1.478 ms per bf16 step, profiles/r06/handoff/).  The re-arm of
// the counter is an agent-scope atomic store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bb {

#ifndef BB_HANDOFF_ORDER
#define BB_HANDOFF_ORDER __ATOMIC_RELEASE  // A/B only: __ATOMIC_RELAXED is the round-5 form (tools/variants.py hrx)
#endif
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) uint32_t guint32;
template <class T>
struct wt_global;
template <>
struct wt_global<float> {
  typedef gfloat type;
};
template <>
struct wt_global<double> {
  typedef gdouble type;
};

template <class T>
__device__ __forceinline__ void wt_store(T* p, T v) {
  __hip_atomic_store((typename wt_global<T>::type*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ T wt_load(const T* p) {
  return __hip_atomic_load((const typename wt_global<T>::type*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// true in the lane whose add completes the count n (it has then acquired every other workgroup's release)
__device__ __forceinline__ bool wt_arrive_last(uint32_t* c, uint32_t n) {
  const bool last = __hip_atomic_fetch_add((guint32*)c, 1u, BB_HANDOFF_ORDER, __HIP_MEMORY_SCOPE_AGENT) == n - 1u;
  if (last && BB_HANDOFF_ORDER != __ATOMIC_RELAXED) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return last;
}
__device__ __forceinline__ void wt_rearm(uint32_t* c) {
  __hip_atomic_store((guint32*)c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the waves' own stores complete before the barrier that precedes the arrive (the release covers them too;
// kept so a wave never reaches the barrier with its partial stores still in flight)
__device__ __forceinline__ void wt_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The tail of a loss kernel of 256 threads, one row per wave, whose waves each hold N fp64 sums (acc, equal in
// all lanes): the waves' sums go to LDS; wave 0 adds them per sum in wave order, publishes the block's N partials
// to part[blockIdx.x][N] and drains them; after a barrier thread 0 counts the block; in the last block to arrive
// lane l of wave k adds blocks l, l + 64, ... for sums k, k + 4, ... (eight loads in flight; the additions in
// block order), and thread 0 adds the 64 lane sums in lane order, calls fin(t) with the N totals and re-arms cnt
// for the next launch.  The order of every addition is fixed, so two launches on the same inputs are
// bit-identical.  Every thread of the block must call it (it holds barriers).  DESIGN.md has the forms measured.
template <int N, class Fin>
__device__ __forceinline__ void block_sums_finish(const double (&acc)[N], double* __restrict__ part, uint32_t* cnt,
                                                  Fin fin) {
  static_assert(N <= 64, "wave 0 publishes one partial per lane");
  __shared__ double red[N][4];
  __shared__ double lsum[N][64];
  __shared__ int last_block;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
    for (int k = 0; k < N; ++k) red[k][w] = acc[k];
  __syncthreads();
  if (threadIdx.x < N) {
    double t = 0.0;
    for (int k = 0; k < 4; ++k) t += red[threadIdx.x][k];
    wt_store(part + (int64_t)blockIdx.x * N + threadIdx.x, t);
    wt_drain();
  }
  __syncthreads();  // wave 0's partial stores have drained
  if (threadIdx.x == 0) last_block = wt_arrive_last(cnt, (uint32_t)gridDim.x);
  __syncthreads();
  if (!last_block) return;
  const int nb = gridDim.x;
  for (int k = w; k < N; k += 4) {
    double t = 0.0;
    for (int b0 = lane; b0 < nb; b0 += 8 * 64) {
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = b0 + 64 * j < nb ? wt_load(part + (int64_t)(b0 + 64 * j) * N + k) : 0.0;
#pragma unroll
      for (int j = 0; j < 8; ++j) t += v[j];
    }
    lsum[k][lane] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[N];
    for (int k = 0; k < N; ++k) {  // unrolled over k: N independent chains, eight LDS reads each in flight
      t[k] = 0.0;
#pragma unroll 8
      for (int l = 0; l < 64; ++l) t[k] += lsum[k][l];
    }
    fin(t);
    wt_rearm(cnt);
  }
}

}  // namespace bb
