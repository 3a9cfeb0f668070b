// bb_loss.hip -- the PPO minibatch loss of PPOAgent.update (ppo.py:362-401)
// with the masked-categorical tail of BlockBlastNetwork (network.py:173-180,
// 210-262), forward and backward, fused (gfx950).
//
// Issued as torch ops the loss is ~45 elementwise / reduction kernels forward
// and as many backward, each a few microseconds on 2,048 x 192 logits; here it
// is one wave per minibatch row, one launch each way (the last block to finish
// finalises the statistics), or one launch for both when the caller supplies
// the loss gradient up front (the graph root's seed: bb_ppo_loss_fused).
//
// The row is bb_loss_rows.h's masked_softmax and ppo_row under the f32 mask (a row with no legal action gets
// no rule of its own here).  Loss = mean(pol) + vcoef * mean(vloss) - ecoef * mean(ent); the statistics (policy /
// value / entropy / total loss, approx_kl, clip_fraction) come from fp64 block partials summed in a fixed order
// (bb_handoff.h block_sums_finish).
#include <hip/hip_runtime.h>

#include "bb_env_internal.h"
#include "bb_handoff.h"
#include "bb_loss_rows.h"

namespace bb {

namespace {

constexpr int kStats = 5;  // partial sums: pol, vloss, ent, kl, clipped

// One wave per row.  STATS: the loss terms' fp64 block partials -> part; with cnt, the last block to arrive adds
// every block's partials and writes stats = [policy_loss, value_loss, entropy, total_loss, approx_kl,
// clip_fraction] and loss = stats[3], re-arming cnt.  GRAD: d loss / d logits, d values for the loss gradient
// gloss[0] (with STATS too, the forward and backward of one minibatch in one launch).
template <bool BF, bool STATS, bool GRAD>
__global__ void __launch_bounds__(kLossThreads) ppo_loss_kernel(
    const void* __restrict__ logits, const void* __restrict__ values, const float* __restrict__ mask,
    const int64_t* __restrict__ actions, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ ret, int B, float clip, float vcoef, float ecoef, const float* __restrict__ gloss,
    void* __restrict__ dlogits, void* __restrict__ dvalues, double* __restrict__ part, uint32_t* cnt,
    float* __restrict__ stats, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const PpoScale k = {clip, 1.f, vcoef, ecoef, GRAD ? gloss[0] : 0.f, 1.f / (float)B};
  for (int64_t row = (int64_t)blockIdx.x * kLossRows + w; row < B; row += (int64_t)gridDim.x * kLossRows) {
    float x[3];
    bool m[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = ld<BF>(logits, row * 192 + j * 64 + lane);
      m[j] = mask[row * 192 + j * 64 + lane] != 0.f;
    }
    const PpoRowIn in = {actions[row], old_logp[row], adv[row], ret[row], ld<BF>(values, row)};
    float dvalue, dz[3];
    ppo_row<STATS, GRAD>(masked_softmax(x, m), m, in, k, lane, acc, dvalue, dz);
    if (GRAD) {
      if (lane == 0) st<BF>(dvalues, row, dvalue);
      st_row<BF>(dlogits, row, lane, dz);
    }
  }
  if (!STATS) return;
  block_sums_finish<kStats>(acc, part, cnt, [&](const double* t) {
    float m[kStats];
    for (int i = 0; i < kStats; ++i) m[i] = (float)(t[i] / (double)B);
    const float total = __fadd_rn(__fadd_rn(m[0], __fmul_rn(vcoef, m[1])), __fmul_rn(ecoef, -m[2]));
    stats[0] = m[0];
    stats[1] = m[1];
    stats[2] = m[2];
    stats[3] = total;
    stats[4] = m[3];
    stats[5] = m[4];
    if (loss) loss[0] = total;
  });
}

}  // namespace

int64_t ppo_loss_workspace_bytes(int B) { return (int64_t)sizeof(double) * kStats * loss_blocks(B); }

// STATS: the forward's half (a.ws, a.cnt, a.stats, a.loss); GRAD: the backward's (a.grad_loss, a.dlogits, a.dvalues)
template <bool STATS, bool GRAD>
hipError_t launch_ppo_loss(const bb_ppo_loss_args& a, hipStream_t s) {
  if (a.B <= 0 || (STATS && !a.cnt)) return hipErrorInvalidValue;
  const auto kernel = a.bf16 ? ppo_loss_kernel<true, STATS, GRAD> : ppo_loss_kernel<false, STATS, GRAD>;
  hipLaunchKernelGGL(kernel, dim3(loss_blocks(a.B)), dim3(kLossThreads), 0, s, a.logits, a.values, a.mask, a.actions,
                     a.old_logp, a.adv, a.ret, a.B, a.clip, a.value_coef, a.entropy_coef, GRAD ? a.grad_loss : nullptr,
                     GRAD ? a.dlogits : nullptr, GRAD ? a.dvalues : nullptr, STATS ? a.ws : nullptr,
                     STATS ? a.cnt : nullptr, STATS ? a.stats : nullptr, STATS ? a.loss : nullptr);
  return hipGetLastError();
}
hipError_t launch_ppo_loss_forward(const bb_ppo_loss_args& a, hipStream_t s) { return launch_ppo_loss<true, false>(a, s); }
hipError_t launch_ppo_loss_backward(const bb_ppo_loss_args& a, hipStream_t s) { return launch_ppo_loss<false, true>(a, s); }
hipError_t launch_ppo_loss_fused(const bb_ppo_loss_args& a, hipStream_t s) { return launch_ppo_loss<true, true>(a, s); }

}  // namespace bb
