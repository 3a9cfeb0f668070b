// bb_guided.hip -- search-guided PPO: the PPO minibatch loss of bb_loss.hip and the distillation cross-entropy of
// bb_distill.hip on one masked softmax, forward and backward, fused (gfx950).
//
//   total = policy_coef * policy_loss + value_coef * value_loss - entropy_coef * entropy + distill_coef * cross_entropy
//
// One wave per minibatch row; bbvec.h "search-guided PPO" has the definitions.  With M the actions whose bit is set
// in mask_bits (the words the policy sampled under; no f32 mask is read), bb_loss_rows.h's masked_softmax runs once
// and both halves use it: ppo_row (the row ppo_loss_kernel runs) and distill_row (the row distill_loss_kernel runs;
// a row with empty S adds nothing to its five sums and gets no distillation gradient; q == NULL: the half is
// skipped, its six statistics are 0).  A row with empty M adds 0 to every sum and its gradients, dvalues included,
// are 0.  The ten row sums go through fp64 block partials that the last block to arrive adds in a fixed order
// (bb_handoff.h block_sums_finish: workspace, one counter re-armed by each launch), so two launches on the same
// inputs are bit-identical.  The five coefficients {policy, value, entropy, distill, tau} come from the arguments
// or, when coefs is non-NULL, from device memory, so a captured step can be replayed under a schedule.
#include <hip/hip_runtime.h>

#include "bb_env_internal.h"
#include "bb_handoff.h"
#include "bb_loss_rows.h"

namespace bb {

namespace {

constexpr int kGuidedSums = 10;  // partial sums: pol, vloss, ent, kl, clipped, ce, ht, hp, agreement, rows

// what a launch reads besides the row tensors: clip and the five coefficients, by value or (coefs) from the device
struct GuidedCoefs {
  float clip, policy, value, entropy, distill, tau;
  const float* dev;  // optional [5] = {policy, value, entropy, distill, tau}
};

}  // namespace

// One wave per row.  STATS: the row sums' fp64 block partials -> part; the last block to arrive adds every
// block's partials and writes stats / loss, re-arming cnt.  GRAD: dlogits and dvalues for the loss gradient
// gloss[0]; with STATS too, forward and backward of one minibatch in one launch.
template <bool BF, bool STATS, bool GRAD>
__global__ void __launch_bounds__(kLossThreads) guided_loss_kernel(
    const void* __restrict__ logits, const void* __restrict__ values, const uint64_t* __restrict__ mask_bits,
    const int64_t* __restrict__ actions, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ ret, const int64_t* __restrict__ q, int B, GuidedCoefs c,
    const float* __restrict__ gloss, void* __restrict__ dlogits, void* __restrict__ dvalues,
    double* __restrict__ part, uint32_t* cnt, float* __restrict__ stats, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float pcoef = c.dev ? c.dev[0] : c.policy, vcoef = c.dev ? c.dev[1] : c.value;
  const float ecoef = c.dev ? c.dev[2] : c.entropy, dcoef = c.dev ? c.dev[3] : c.distill;
  const float tau = c.dev ? c.dev[4] : c.tau;
  double acc[kGuidedSums];
#pragma unroll
  for (int k = 0; k < kGuidedSums; ++k) acc[k] = 0.0;
  const PpoScale k = {c.clip, pcoef, vcoef, ecoef, GRAD ? gloss[0] : 0.f, 1.f / (float)B};
  const float dscale = GRAD ? __fdiv_rn(__fmul_rn(k.g, dcoef), (float)B) : 0.f;
  for (int64_t row = (int64_t)blockIdx.x * kLossRows + w; row < B; row += (int64_t)gridDim.x * kLossRows) {
    float x[3];
    bool m[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = ld<BF>(logits, row * 192 + j * 64 + lane);
      m[j] = (mask_bits[row * 3 + j] >> lane) & 1ull;
    }
    float dvalue = 0.f, dz[3] = {0.f, 0.f, 0.f};
    if (ballot3(m[0], m[1], m[2]).any()) {  // empty M (the whole wave): nothing
      const Softmax sm = masked_softmax(x, m);
      float dg[3] = {0.f, 0.f, 0.f};
      if (q != nullptr) {
        int64_t qv[3];
        bool s[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          qv[j] = q[row * 192 + j * 64 + lane];
          s[j] = m[j] && qv[j] != INT64_MIN;
        }
        if (ballot3(s[0], s[1], s[2]).any())  // non-empty S (the whole wave)
          distill_row<STATS, GRAD>(x, m, s, qv, sm.mx, sm.se, tau, dscale, lane, acc + 5, dg);
      }
      const PpoRowIn in = {actions[row], old_logp[row], adv[row], ret[row], ld<BF>(values, row)};
      ppo_row<STATS, GRAD>(sm, m, in, k, lane, acc, dvalue, dz);
      if (GRAD) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dz[j] = m[j] ? __fadd_rn(dz[j], dg[j]) : 0.f;  // outside M: p = 0 and dg = 0
      }
    }
    if (GRAD) {
      if (lane == 0) st<BF>(dvalues, row, dvalue);
      st_row<BF>(dlogits, row, lane, dz);
    }
  }
  if (!STATS) return;
  block_sums_finish<kGuidedSums>(acc, part, cnt, [&](const double* t) {
    const double b = (double)B;
    float mean[5];
    for (int i = 0; i < 5; ++i) mean[i] = (float)(t[i] / b);
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
  });
}

namespace {
// STATS: the forward's half (a.ws, a.cnt, a.stats, a.loss); GRAD: the backward's (a.grad_loss, a.dlogits, a.dvalues)
template <bool STATS, bool GRAD>
hipError_t launch_guided_loss(const bb_guided_loss_args& a, hipStream_t s) {
  if (a.B <= 0 || (STATS && !a.cnt)) return hipErrorInvalidValue;
  const auto kernel = a.bf16 ? guided_loss_kernel<true, STATS, GRAD> : guided_loss_kernel<false, STATS, GRAD>;
  const GuidedCoefs c = {a.clip, a.policy_coef, a.value_coef, a.entropy_coef, a.distill_coef, a.tau, a.coefs_dev};
  hipLaunchKernelGGL(kernel, dim3(loss_blocks(a.B)), dim3(kLossThreads), 0, s, a.logits, a.values, a.mask_bits,
                     a.actions, a.old_logp, a.adv, a.ret, a.q, a.B, c, GRAD ? a.grad_loss : nullptr,
                     GRAD ? a.dlogits : nullptr, GRAD ? a.dvalues : nullptr, STATS ? a.ws : nullptr,
                     STATS ? a.cnt : nullptr, STATS ? a.stats : nullptr, STATS ? a.loss : nullptr);
  return hipGetLastError();
}
}  // namespace

int64_t guided_loss_workspace_bytes(int B) { return (int64_t)sizeof(double) * kGuidedSums * loss_blocks(B); }
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
