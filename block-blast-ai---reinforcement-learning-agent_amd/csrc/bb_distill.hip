// bb_distill.hip -- policy distillation from the full-hand search: the cross-entropy between a softmax over
// bb_plan_values' per-action values and the masked policy, forward and backward, fused (gfx950).
//
// One wave per minibatch row, 3 entries per lane (action j * 64 + lane), the layout of ppo_loss_kernel and
// masked_sample_kernel.  Per row (fp32; bbvec.h "policy distillation" has the definitions):
//   M      = the actions whose bit is set in mask_bits (the words the policy sampled under)
//   S      = the a in M with q[a] != INT64_MIN;  qmax = max q over S
//   t      = softmax over S of float(q - qmax) / tau (the difference in int64, exact; below -2^31: 0), or with
//            tau == 0 the one-hot of the lowest a attaining qmax (bb_plan_actions' action)
//   logpi  = log_softmax(logits + where(M, 0, -inf)) by max-subtraction, no clamp;  pi = exp(logpi)
//   ce     = -sum_{t > 0} t logpi      ht = -sum_{t > 0} t log t      hp = -sum_M pi logpi
//   agree  = [lowest argmax of the logits over M == lowest argmax of q over S]
// A row with empty S adds nothing to any sum and gets zero gradients.  stats = {ce, ce - ht, ht, hp, agree} / B
// and the number of rows with non-empty S, from fp64 block partials that the last block to arrive adds in a
// fixed order (the hand-off of bb_loss.hip: workspace, one counter re-armed by each launch), so two launches on
// the same inputs are bit-identical.  Backward: dlogits = grad_loss / B (pi - t) on M, 0 elsewhere.  Logits may
// be bf16: widened exactly on load, their gradient rounded to nearest even on store.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>
#include <stdint.h>

#include "bb_env_internal.h"

namespace bb {

namespace {

constexpr int kDistillThreads = 256;
constexpr int kDistillRows = kDistillThreads / 64;  // rows (waves) per block
constexpr int kDistillSums = 5;                     // partial sums: ce, ht, hp, agreement, rows

__device__ __forceinline__ float dmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float dsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int64_t dmax64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t u = (int64_t)__shfl_xor((long long)v, o);
    v = u > v ? u : v;
  }
  return v;
}
// the lowest action whose bit is set in the three ballots (word j = actions j * 64 ...), -1 if none
__device__ __forceinline__ int lowest(uint64_t b0, uint64_t b1, uint64_t b2) {
  if (b0) return __builtin_ctzll(b0);
  if (b1) return 64 + __builtin_ctzll(b1);
  if (b2) return 128 + __builtin_ctzll(b2);
  return -1;
}

template <bool BF>
__device__ __forceinline__ float ldl(const void* __restrict__ p, int64_t i) {
  if constexpr (BF) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
  return reinterpret_cast<const float*>(p)[i];
}
template <bool BF>
__device__ __forceinline__ void stl(void* __restrict__ p, int64_t i, float v) {
  if constexpr (BF) {
    const __hip_bfloat16 b = __float2bfloat16(v);  // round to nearest even, as torch's cast
    reinterpret_cast<uint16_t*>(p)[i] = *reinterpret_cast<const uint16_t*>(&b);
  } else {
    reinterpret_cast<float*>(p)[i] = v;
  }
}

typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) uint32_t guint32;

}  // namespace

// One wave per row.  STATS: the row sums' fp64 block partials -> part; the last block to arrive adds every
// block's partials (lanes, then waves, in a fixed order) and writes stats / loss, re-arming cnt.  GRAD: dlogits
// for the loss gradient gloss[0]; with STATS too, forward and backward of one minibatch in one launch.
template <bool BF, bool STATS, bool GRAD>
__global__ void __launch_bounds__(kDistillThreads) distill_loss_kernel(
    const void* __restrict__ logits, const uint64_t* __restrict__ mask_bits, const int64_t* __restrict__ q, int B,
    float tau, const float* __restrict__ gloss, void* __restrict__ dlogits, double* __restrict__ part, uint32_t* cnt,
    float* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double red[kDistillSums][kDistillRows];
  __shared__ int last_block;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[kDistillSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const float scale = GRAD ? __fdiv_rn(gloss[0], (float)B) : 0.f;
  for (int64_t row = (int64_t)blockIdx.x * kDistillRows + w; row < B; row += (int64_t)gridDim.x * kDistillRows) {
    float x[3];
    int64_t qv[3];
    bool m[3], s[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = ldl<BF>(logits, row * 192 + j * 64 + lane);
      qv[j] = q[row * 192 + j * 64 + lane];
      m[j] = (mask_bits[row * 3 + j] >> lane) & 1ull;
      s[j] = m[j] && qv[j] != INT64_MIN;
    }
    if ((__ballot(s[0]) | __ballot(s[1]) | __ballot(s[2])) == 0ull) {  // empty S (the whole wave): nothing
      if (GRAD) {
#pragma unroll
        for (int j = 0; j < 3; ++j) stl<BF>(dlogits, row * 192 + j * 64 + lane, 0.f);
      }
      continue;
    }
    // the student: log-softmax over M
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (m[j]) mx = fmaxf(mx, x[j]);
    mx = dmax(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) se = __fadd_rn(se, m[j] ? expf(__fsub_rn(x[j], mx)) : 0.f);
    const float lse = logf(dsum(se));
    float logpi[3], pi[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      logpi[j] = m[j] ? __fsub_rn(__fsub_rn(x[j], mx), lse) : 0.f;
      pi[j] = m[j] ? expf(logpi[j]) : 0.f;
    }
    // the teacher: softmax over S of (q - qmax) / tau, or the lowest argmax
    int64_t qm = INT64_MIN;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (s[j] && qv[j] > qm) qm = qv[j];
    qm = dmax64(qm);
    const int qarg = lowest(__ballot(s[0] && qv[0] == qm), __ballot(s[1] && qv[1] == qm), __ballot(s[2] && qv[2] == qm));
    float t[3];
    if (tau > 0.f) {
      float wt[3], z = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int64_t d = s[j] ? qv[j] - qm : 0;  // <= 0, exact
        wt[j] = (s[j] && d >= -2147483648ll) ? expf(__fdiv_rn((float)d, tau)) : 0.f;
        z = __fadd_rn(z, wt[j]);
      }
      z = dsum(z);  // >= 1: the maximum's weight is 1
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = __fdiv_rn(wt[j], z);
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = j * 64 + lane == qarg ? 1.f : 0.f;
    }
    if (STATS) {
      float ce = 0.f, ht = 0.f, hp = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        ce = __fadd_rn(ce, t[j] > 0.f ? __fmul_rn(t[j], logpi[j]) : 0.f);
        ht = __fadd_rn(ht, t[j] > 0.f ? __fmul_rn(t[j], logf(t[j])) : 0.f);
        hp = __fadd_rn(hp, pi[j] > 0.f ? __fmul_rn(pi[j], logpi[j]) : 0.f);
      }
      ce = dsum(ce);
      ht = dsum(ht);
      hp = dsum(hp);
      const int parg = lowest(__ballot(m[0] && x[0] == mx), __ballot(m[1] && x[1] == mx), __ballot(m[2] && x[2] == mx));
      acc[0] += (double)-ce;
      acc[1] += (double)-ht;
      acc[2] += (double)-hp;
      acc[3] += parg == qarg ? 1.0 : 0.0;
      acc[4] += 1.0;
    }
    if (GRAD) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        stl<BF>(dlogits, row * 192 + j * 64 + lane, m[j] ? __fmul_rn(scale, __fsub_rn(pi[j], t[j])) : 0.f);
    }
  }
  if (!STATS) return;
  if (lane == 0)
    for (int k = 0; k < kDistillSums; ++k) red[k][w] = acc[k];
  __syncthreads();
  // Wave 0 publishes the block's partials and counts the block (the hand-off of bb_loss.hip, ordered by the HIP
  // memory model alone): agent-scope stores (written through), then lane 0's agent-scope release add, whose
  // write-back and wait on this wave's outstanding stores come before the add.  The lane whose add returns the
  // last count issues an agent-scope acquire fence; its block, after the barrier, reads every partial with
  // agent-scope loads, finalises and re-arms the counter.
  if (w == 0) {
    if (lane < kDistillSums) {
      double t = 0.0;
      for (int k = 0; k < kDistillRows; ++k) t += red[lane][k];
      __hip_atomic_store((gdouble*)(part + (int64_t)blockIdx.x * kDistillSums + lane), t, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) {
      const bool last = __hip_atomic_fetch_add((guint32*)cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT) ==
                        (uint32_t)gridDim.x - 1u;
      if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      last_block = last;
    }
  }
  __syncthreads();
  if (!last_block) return;
  // lane l of wave k adds blocks l, l + 64, ... for sum k (wave 0 then takes sum 4), the lanes' sums in lane
  // order through LDS
  __shared__ double lsum[kDistillSums][64];
  const int nb = gridDim.x;
  for (int k = w; k < kDistillSums; k += kDistillRows) {
    double t = 0.0;
#pragma unroll 4
    for (int b = lane; b < nb; b += 64)
      t += __hip_atomic_load((const gdouble*)(part + (int64_t)b * kDistillSums + k), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    lsum[k][lane] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[kDistillSums];
    for (int k = 0; k < kDistillSums; ++k) {
      t[k] = 0.0;
#pragma unroll 8
      for (int l = 0; l < 64; ++l) t[k] += lsum[k][l];
    }
    const double b = (double)B;
    stats[0] = (float)(t[0] / b);
    stats[1] = (float)((t[0] - t[1]) / b);
    stats[2] = (float)(t[1] / b);
    stats[3] = (float)(t[2] / b);
    stats[4] = (float)(t[3] / b);
    stats[5] = (float)t[4];
    if (loss) loss[0] = stats[0];
    __hip_atomic_store((guint32*)cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
  }
}

namespace {
int distill_blocks(int B) {
  const int b = (B + kDistillRows - 1) / kDistillRows;
  return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

// STATS: the forward's half (a.ws, a.cnt, a.stats, a.loss); GRAD: the backward's (a.grad_loss, a.dlogits)
template <bool STATS, bool GRAD>
hipError_t launch_distill_loss(const bb_distill_loss_args& a, hipStream_t s) {
  if (a.B <= 0 || (STATS && !a.cnt)) return hipErrorInvalidValue;
  const auto kernel = a.bf16 ? distill_loss_kernel<true, STATS, GRAD> : distill_loss_kernel<false, STATS, GRAD>;
  hipLaunchKernelGGL(kernel, dim3(distill_blocks(a.B)), dim3(kDistillThreads), 0, s, a.logits, a.mask_bits, a.q, a.B,
                     a.tau, GRAD ? a.grad_loss : nullptr, GRAD ? a.dlogits : nullptr, STATS ? a.ws : nullptr,
                     STATS ? a.cnt : nullptr, STATS ? a.stats : nullptr, STATS ? a.loss : nullptr);
  return hipGetLastError();
}
}  // namespace

int64_t distill_loss_workspace_bytes(int B) { return (int64_t)sizeof(double) * kDistillSums * distill_blocks(B); }
hipError_t launch_distill_loss_forward(const bb_distill_loss_args& a, hipStream_t s) {
  return launch_distill_loss<true, false>(a, s);
}
hipError_t launch_distill_loss_backward(const bb_distill_loss_args& a, hipStream_t s) {
  return launch_distill_loss<false, true>(a, s);
}
hipError_t launch_distill_loss_fused(const bb_distill_loss_args& a, hipStream_t s) {
  return launch_distill_loss<true, true>(a, s);
}

}  // namespace bb
