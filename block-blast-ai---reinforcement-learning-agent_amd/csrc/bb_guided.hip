// bb_guided.hip -- search-guided PPO: the PPO minibatch loss of bb_loss.hip and the distillation cross-entropy of
// bb_distill.hip on one masked softmax, forward and backward, fused (gfx950).
//
//   total = policy_coef * policy_loss + value_coef * value_loss - entropy_coef * entropy + distill_coef * cross_entropy
//
// One wave per minibatch row, 3 entries per lane (action j * 64 + lane), the layout of ppo_loss_kernel and
// distill_loss_kernel.  Per row (fp32; bbvec.h "search-guided PPO" has the definitions), with M the actions whose
// bit is set in mask_bits (the words the policy sampled under; no f32 mask is read):
//   mx, se = the maximum of the logits over M and the sum over M of exp(x - mx): computed once, used by both halves
//   PPO    = ppo_loss_kernel's row with the mask taken as M: p = e / se, P = p / sum p, logp = log(clamp(P[a], eps,
//            1 - eps)), the masked entropy with its 1e-10 clamps, ratio, clipped surrogate, (v - ret)^2, approx_kl,
//            clip_fraction; backward by autograd's rules for min (ties half/half), clamp (closed interval) and log
//   distil = distill_loss_kernel's row: S = the a in M with q[a] != INT64_MIN, qmax, t = softmax over S of
//            float(q - qmax) / tau (int64 difference; below -2^31: 0) or at tau == 0 the one-hot of the lowest
//            argmax, logpi = (x - mx) - log(se), pi = exp(logpi), ce, ht, hp, agree, rows; a row with empty S adds
//            nothing to these five and gets no distillation gradient.  q == NULL: the half is skipped, its six
//            statistics are 0.
// A row with empty M adds 0 to every sum and its gradients, dvalues included, are 0.  The ten row sums go through
// fp64 block partials that the last block to arrive adds in a fixed order (the hand-off of bb_distill.hip: workspace,
// one counter re-armed by each launch), so two launches on the same inputs are bit-identical.  The five
// coefficients {policy, value, entropy, distill, tau} come from the arguments or, when coefs is non-NULL, from
// device memory, so a captured step can be replayed under a schedule.  Logits and values may be bf16: widened
// exactly on load, their gradients rounded to nearest even on store.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>
#include <stdint.h>

#include "bb_env_internal.h"

namespace bb {

namespace {

constexpr int kGuidedThreads = 256;
constexpr int kGuidedRows = kGuidedThreads / 64;  // rows (waves) per block
constexpr int kGuidedSums = 10;  // partial sums: pol, vloss, ent, kl, clipped, ce, ht, hp, agreement, rows
constexpr float kGuidedEps32 = 1.1920928955078125e-07f;  // torch.finfo(float32).eps

__device__ __forceinline__ float gmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float gsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int64_t gmax64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t u = (int64_t)__shfl_xor((long long)v, o);
    v = u > v ? u : v;
  }
  return v;
}
// the lowest action whose bit is set in the three ballots (word j = actions j * 64 ...), -1 if none
__device__ __forceinline__ int glowest(uint64_t b0, uint64_t b1, uint64_t b2) {
  if (b0) return __builtin_ctzll(b0);
  if (b1) return 64 + __builtin_ctzll(b1);
  if (b2) return 128 + __builtin_ctzll(b2);
  return -1;
}

template <bool BF>
__device__ __forceinline__ float ldg(const void* __restrict__ p, int64_t i) {
  if constexpr (BF) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
  return reinterpret_cast<const float*>(p)[i];
}
template <bool BF>
__device__ __forceinline__ void stg(void* __restrict__ p, int64_t i, float v) {
  if constexpr (BF) {
    const __hip_bfloat16 b = __float2bfloat16(v);  // round to nearest even, as torch's cast
    reinterpret_cast<uint16_t*>(p)[i] = *reinterpret_cast<const uint16_t*>(&b);
  } else {
    reinterpret_cast<float*>(p)[i] = v;
  }
}

typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) uint32_t guint32;

// what a launch reads besides the row tensors: clip and the five coefficients, by value or (coefs) from the device
struct GuidedCoefs {
  float clip, policy, value, entropy, distill, tau;
  const float* dev;  // optional [5] = {policy, value, entropy, distill, tau}
};

}  // namespace

// One wave per row.  STATS: the row sums' fp64 block partials -> part; the last block to arrive adds every
// block's partials (lanes, then waves, in a fixed order) and writes stats / loss, re-arming cnt.  GRAD: dlogits
// and dvalues for the loss gradient gloss[0]; with STATS too, forward and backward of one minibatch in one launch.
template <bool BF, bool STATS, bool GRAD>
__global__ void __launch_bounds__(kGuidedThreads) guided_loss_kernel(
    const void* __restrict__ logits, const void* __restrict__ values, const uint64_t* __restrict__ mask_bits,
    const int64_t* __restrict__ actions, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ ret, const int64_t* __restrict__ q, int B, GuidedCoefs c,
    const float* __restrict__ gloss, void* __restrict__ dlogits, void* __restrict__ dvalues,
    double* __restrict__ part, uint32_t* cnt, float* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double red[kGuidedSums][kGuidedRows];
  __shared__ int last_block;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float clip = c.clip;
  const float pcoef = c.dev ? c.dev[0] : c.policy, vcoef = c.dev ? c.dev[1] : c.value;
  const float ecoef = c.dev ? c.dev[2] : c.entropy, dcoef = c.dev ? c.dev[3] : c.distill;
  const float tau = c.dev ? c.dev[4] : c.tau;
  double acc[kGuidedSums];
#pragma unroll
  for (int k = 0; k < kGuidedSums; ++k) acc[k] = 0.0;
  const float g = GRAD ? gloss[0] : 0.f;
  const float invB = 1.f / (float)B;
  const float dscale = GRAD ? __fdiv_rn(__fmul_rn(g, dcoef), (float)B) : 0.f;
  for (int64_t row = (int64_t)blockIdx.x * kGuidedRows + w; row < B; row += (int64_t)gridDim.x * kGuidedRows) {
    float x[3];
    bool m[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = ldg<BF>(logits, row * 192 + j * 64 + lane);
      m[j] = (mask_bits[row * 3 + j] >> lane) & 1ull;
    }
    if ((__ballot(m[0]) | __ballot(m[1]) | __ballot(m[2])) == 0ull) {  // empty M (the whole wave): nothing
      if (GRAD) {
#pragma unroll
        for (int j = 0; j < 3; ++j) stg<BF>(dlogits, row * 192 + j * 64 + lane, 0.f);
        if (lane == 0) stg<BF>(dvalues, row, 0.f);
      }
      continue;
    }
    // the masked softmax both halves share: the row maximum, the exponentials and their sum
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (m[j]) mx = fmaxf(mx, x[j]);
    mx = gmax(mx);
    float e[3], se = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      e[j] = m[j] ? expf(__fsub_rn(x[j], mx)) : 0.f;
      se = __fadd_rn(se, e[j]);
    }
    se = gsum(se);

    // ---- the distillation half (distill_loss_kernel's row): its gradient dg, its five sums
    float dg[3] = {0.f, 0.f, 0.f};
    if (q != nullptr) {
      int64_t qv[3];
      bool s[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        qv[j] = q[row * 192 + j * 64 + lane];
        s[j] = m[j] && qv[j] != INT64_MIN;
      }
      if ((__ballot(s[0]) | __ballot(s[1]) | __ballot(s[2])) != 0ull) {  // non-empty S (the whole wave)
        const float lse = logf(se);
        float logpi[3], pi[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          logpi[j] = m[j] ? __fsub_rn(__fsub_rn(x[j], mx), lse) : 0.f;
          pi[j] = m[j] ? expf(logpi[j]) : 0.f;
        }
        int64_t qm = INT64_MIN;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (s[j] && qv[j] > qm) qm = qv[j];
        qm = gmax64(qm);
        const int qarg =
            glowest(__ballot(s[0] && qv[0] == qm), __ballot(s[1] && qv[1] == qm), __ballot(s[2] && qv[2] == qm));
        float t[3];
        if (tau > 0.f) {
          float wt[3], z = 0.f;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int64_t d = s[j] ? qv[j] - qm : 0;  // <= 0, exact
            wt[j] = (s[j] && d >= -2147483648ll) ? expf(__fdiv_rn((float)d, tau)) : 0.f;
            z = __fadd_rn(z, wt[j]);
          }
          z = gsum(z);  // >= 1: the maximum's weight is 1
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
          ce = gsum(ce);
          ht = gsum(ht);
          hp = gsum(hp);
          const int parg =
              glowest(__ballot(m[0] && x[0] == mx), __ballot(m[1] && x[1] == mx), __ballot(m[2] && x[2] == mx));
          acc[5] += (double)-ce;
          acc[6] += (double)-ht;
          acc[7] += (double)-hp;
          acc[8] += parg == qarg ? 1.0 : 0.0;
          acc[9] += 1.0;
        }
        if (GRAD) {
#pragma unroll
          for (int j = 0; j < 3; ++j) dg[j] = m[j] ? __fmul_rn(dscale, __fsub_rn(pi[j], t[j])) : 0.f;
        }
      }
    }

    // ---- the PPO half (ppo_loss_kernel's row with the mask taken as M)
    const int64_t a = actions[row];
    const int aj = (int)(a >> 6), al = (int)(a & 63);
    float p[3], s0 = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      p[j] = __fdiv_rn(e[j], se);
      s0 = __fadd_rn(s0, p[j]);
    }
    const float sp = gsum(s0);  // sum of p
    const float p_a = __shfl(aj == 0 ? p[0] : (aj == 1 ? p[1] : p[2]), al);
    const float pa = __fdiv_rn(p_a, sp);  // P[a]
    const float logp = logf(fminf(fmaxf(pa, kGuidedEps32), 1.f - kGuidedEps32));
    float ms0 = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) ms0 = __fadd_rn(ms0, m[j] ? p[j] : 0.f);
    const float ms_raw = gsum(ms0);
    const float ms = fmaxf(ms_raw, 1e-10f);
    float qn[3], lq[3], h = 0.f;  // masked p / ms and its clamped logarithm
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      qn[j] = __fdiv_rn(m[j] ? p[j] : 0.f, ms);
      lq[j] = logf(fmaxf(qn[j], 1e-10f));
      h = __fadd_rn(h, m[j] ? __fmul_rn(qn[j], lq[j]) : 0.f);
    }
    const float ent = -gsum(h);
    const float A = adv[row];
    const float ratio = expf(__fsub_rn(logp, old_logp[row]));
    const float s1 = __fmul_rn(ratio, A), s2 = __fmul_rn(fminf(fmaxf(ratio, 1.f - clip), 1.f + clip), A);
    const float dv = __fsub_rn(ldg<BF>(values, row), ret[row]);
    if (STATS) {
      const float rm1 = __fsub_rn(ratio, 1.f);
      acc[0] += (double)(-fminf(s1, s2));
      acc[1] += (double)__fmul_rn(dv, dv);
      acc[2] += (double)ent;
      acc[3] += (double)__fsub_rn(rm1, logf(ratio));
      acc[4] += fabsf(rm1) > clip ? 1.0 : 0.0;
    }
    if (GRAD) {
      // d loss / d min(s1, s2) = -g policy_coef / B; torch.min splits ties half/half
      const float gmin = -(g * pcoef) * invB;
      const float g1 = s1 < s2 ? gmin : (s1 > s2 ? 0.f : 0.5f * gmin);
      const float g2 = s2 < s1 ? gmin : (s2 > s1 ? 0.f : 0.5f * gmin);
      const bool in_clip = ratio >= 1.f - clip && ratio <= 1.f + clip;
      const float glogp = (g1 * A + (in_clip ? g2 * A : 0.f)) * ratio;  // d exp(x)/dx = exp(x)
      if (lane == 0) stg<BF>(dvalues, row, vcoef * g * invB * 2.f * dv);  // mse
      const float gent = -ecoef * g * invB;  // entropy_coef * (-mean(ent))
      // log(clamp(P_a, eps, 1 - eps)): passes where eps <= P_a <= 1 - eps, divided by the clamped value
      const float gPa = (pa >= kGuidedEps32 && pa <= 1.f - kGuidedEps32) ? glogp / pa : 0.f;
      // P = p / s: gp_k = [k == a] gPa / s - gPa p_a / s^2
      const float corr = gPa * p_a / (sp * sp);
      // entropy = -sum m q log(clamp(q, 1e-10)), q = m p / clamp(ms, 1e-10):
      //   d/dq_j = -m_j (log(clamp(q_j)) + [q_j >= 1e-10])
      float gq[3], sgqm = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        gq[j] = m[j] ? -gent * (lq[j] + (qn[j] >= 1e-10f ? 1.f : 0.f)) : 0.f;
        sgqm += m[j] ? gq[j] * p[j] : 0.f;
      }
      sgqm = gsum(sgqm);
      const float gms = ms_raw >= 1e-10f ? -sgqm / (ms * ms) : 0.f;
      float gp[3], dot = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        gp[j] = ((j == aj && lane == al) ? gPa / sp : 0.f) - corr;
        if (m[j]) gp[j] += gq[j] / ms + gms;
        dot += gp[j] * p[j];
      }
      dot = gsum(dot);
      // softmax backward: dz_k = p_k (gp_k - sum_j gp_j p_j); entries outside M have p = 0 and dg = 0
#pragma unroll
      for (int j = 0; j < 3; ++j)
        stg<BF>(dlogits, row * 192 + j * 64 + lane, m[j] ? __fadd_rn(p[j] * (gp[j] - dot), dg[j]) : 0.f);
    }
  }
  if (!STATS) return;
  if (lane == 0)
    for (int k = 0; k < kGuidedSums; ++k) red[k][w] = acc[k];
  __syncthreads();
  // Wave 0 publishes the block's partials and counts the block (the hand-off of bb_distill.hip, ordered by the HIP
  // memory model alone): agent-scope stores (written through), then lane 0's agent-scope release add, whose
  // write-back and wait on this wave's outstanding stores come before the add.  The lane whose add returns the
  // last count issues an agent-scope acquire fence; its block, after the barrier, reads every partial with
  // agent-scope loads, finalises and re-arms the counter.
  if (w == 0) {
    if (lane < kGuidedSums) {
      double t = 0.0;
      for (int k = 0; k < kGuidedRows; ++k) t += red[lane][k];
      __hip_atomic_store((gdouble*)(part + (int64_t)blockIdx.x * kGuidedSums + lane), t, __ATOMIC_RELAXED,
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
  // lane l of wave k adds blocks l, l + 64, ... for sums k, k + 4, k + 8, the lanes' sums in lane order through LDS
  __shared__ double lsum[kGuidedSums][64];
  const int nb = gridDim.x;
  for (int k = w; k < kGuidedSums; k += kGuidedRows) {
    double t = 0.0;
#pragma unroll 4
    for (int b = lane; b < nb; b += 64)
      t += __hip_atomic_load((const gdouble*)(part + (int64_t)b * kGuidedSums + k), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    lsum[k][lane] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[kGuidedSums];
#pragma unroll 1
    for (int k = 0; k < kGuidedSums; ++k) {
      t[k] = 0.0;
#pragma unroll 8
      for (int l = 0; l < 64; ++l) t[k] += lsum[k][l];
    }
    const double b = (double)B;
    float mean[5];
    for (int k = 0; k < 5; ++k) mean[k] = (float)(t[k] / b);
    const float ce = (float)(t[5] / b);
    const float total = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(pcoef, mean[0]), __fmul_rn(vcoef, mean[1])),
                                            __fmul_rn(ecoef, -mean[2])),
                                  __fmul_rn(dcoef, ce));
    stats[0] = mean[0];
    stats[1] = mean[1];
    stats[2] = mean[2];
    stats[3] = total;
    stats[4] = mean[3];
    stats[5] = mean[4];
    stats[6] = ce;
    stats[7] = (float)((t[5] - t[6]) / b);
    stats[8] = (float)(t[6] / b);
    stats[9] = (float)(t[7] / b);
    stats[10] = (float)(t[8] / b);
    stats[11] = (float)t[9];
    if (loss) loss[0] = total;
    __hip_atomic_store((guint32*)cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
  }
}

namespace {
int guided_blocks(int B) {
  const int b = (B + kGuidedRows - 1) / kGuidedRows;
  return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

// STATS: the forward's half (a.ws, a.cnt, a.stats, a.loss); GRAD: the backward's (a.grad_loss, a.dlogits, a.dvalues)
template <bool STATS, bool GRAD>
hipError_t launch_guided_loss(const bb_guided_loss_args& a, hipStream_t s) {
  if (a.B <= 0 || (STATS && !a.cnt)) return hipErrorInvalidValue;
  const auto kernel = a.bf16 ? guided_loss_kernel<true, STATS, GRAD> : guided_loss_kernel<false, STATS, GRAD>;
  const GuidedCoefs c = {a.clip, a.policy_coef, a.value_coef, a.entropy_coef, a.distill_coef, a.tau, a.coefs_dev};
  hipLaunchKernelGGL(kernel, dim3(guided_blocks(a.B)), dim3(kGuidedThreads), 0, s, a.logits, a.values, a.mask_bits,
                     a.actions, a.old_logp, a.adv, a.ret, a.q, a.B, c, GRAD ? a.grad_loss : nullptr,
                     GRAD ? a.dlogits : nullptr, GRAD ? a.dvalues : nullptr, STATS ? a.ws : nullptr,
                     STATS ? a.cnt : nullptr, STATS ? a.stats : nullptr, STATS ? a.loss : nullptr);
  return hipGetLastError();
}
}  // namespace

int64_t guided_loss_workspace_bytes(int B) { return (int64_t)sizeof(double) * kGuidedSums * guided_blocks(B); }
hipError_t launch_guided_loss_forward(const bb_guided_loss_args& a, hipStream_t s) {
  return launch_guided_loss<true, false>(a, s);
}
hipError_t launch_guided_loss_backward(const bb_guided_loss_args& a, hipStream_t s) {
  return launch_guided_loss<false, true>(a, s);
}
hipError_t launch_guided_loss_fused(const bb_guided_loss_args& a, hipStream_t s) {
  return launch_guided_loss<true, true>(a, s);
}

}  // namespace bb
