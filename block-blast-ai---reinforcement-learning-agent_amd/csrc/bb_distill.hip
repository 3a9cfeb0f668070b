// bb_distill.hip -- policy distillation from the full-hand search: the cross-entropy between a softmax over
// bb_plan_values' per-action values and the masked policy, forward and backward, fused (gfx950).
//
// One wave per minibatch row; the row is bb_loss_rows.h's masked_softmax and distill_row under M = the actions
// whose bit is set in mask_bits (the words the policy sampled under); bbvec.h "policy distillation" has the
// definitions.  A row with empty S adds nothing to any sum and gets zero gradients.  stats = {ce, ce - ht, ht, hp,
// agree} / B and the number of rows with non-empty S, from fp64 block partials that the last block to arrive adds
// in a fixed order (bb_handoff.h block_sums_finish: workspace, one counter re-armed by each launch), so two
// launches on the same inputs are bit-identical.  Backward: dlogits = grad_loss / B (pi - t) on M, 0 elsewhere.
#include <hip/hip_runtime.h>

#include "bb_env_internal.h"
#include "bb_handoff.h"
#include "bb_loss_rows.h"

namespace bb {

namespace {
constexpr int kDistillSums = 5;  // partial sums: ce, ht, hp, agreement, rows
}  // namespace

// One wave per row.  STATS: the row sums' fp64 block partials -> part; the last block to arrive adds every
// block's partials and writes stats / loss, re-arming cnt.  GRAD: dlogits for the loss gradient gloss[0]; with
// STATS too, forward and backward of one minibatch in one launch.
template <bool BF, bool STATS, bool GRAD>
__global__ void __launch_bounds__(kLossThreads) distill_loss_kernel(
    const void* __restrict__ logits, const uint64_t* __restrict__ mask_bits, const int64_t* __restrict__ q, int B,
    float tau, const float* __restrict__ gloss, void* __restrict__ dlogits, double* __restrict__ part, uint32_t* cnt,
    float* __restrict__ stats, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[kDistillSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const float scale = GRAD ? __fdiv_rn(gloss[0], (float)B) : 0.f;
  for (int64_t row = (int64_t)blockIdx.x * kLossRows + w; row < B; row += (int64_t)gridDim.x * kLossRows) {
    float x[3];
    int64_t qv[3];
    bool m[3], s[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = ld<BF>(logits, row * 192 + j * 64 + lane);
      qv[j] = q[row * 192 + j * 64 + lane];
      m[j] = (mask_bits[row * 3 + j] >> lane) & 1ull;
      s[j] = m[j] && qv[j] != INT64_MIN;
    }
    float dg[3] = {0.f, 0.f, 0.f};
    if (ballot3(s[0], s[1], s[2]).any()) {  // empty S (the whole wave): nothing
      const Softmax sm = masked_softmax(x, m);
      distill_row<STATS, GRAD>(x, m, s, qv, sm.mx, sm.se, tau, scale, lane, acc, dg);
    }
    if (GRAD) st_row<BF>(dlogits, row, lane, dg);
  }
  if (!STATS) return;
  block_sums_finish<kDistillSums>(acc, part, cnt, [&](const double* t) {
    const double b = (double)B;
    stats[0] = (float)(t[0] / b);
    stats[1] = (float)((t[0] - t[1]) / b);
    stats[2] = (float)(t[1] / b);
    stats[3] = (float)(t[2] / b);
    stats[4] = (float)(t[3] / b);
    stats[5] = (float)t[4];
    if (loss) loss[0] = stats[0];
  });
}

namespace {
// STATS: the forward's half (a.ws, a.cnt, a.stats, a.loss); GRAD: the backward's (a.grad_loss, a.dlogits)
template <bool STATS, bool GRAD>
hipError_t launch_distill_loss(const bb_distill_loss_args& a, hipStream_t s) {
  if (a.B <= 0 || (STATS && !a.cnt)) return hipErrorInvalidValue;
  const auto kernel = a.bf16 ? distill_loss_kernel<true, STATS, GRAD> : distill_loss_kernel<false, STATS, GRAD>;
  hipLaunchKernelGGL(kernel, dim3(loss_blocks(a.B)), dim3(kLossThreads), 0, s, a.logits, a.mask_bits, a.q, a.B,
                     a.tau, GRAD ? a.grad_loss : nullptr, GRAD ? a.dlogits : nullptr, STATS ? a.ws : nullptr,
                     STATS ? a.cnt : nullptr, STATS ? a.stats : nullptr, STATS ? a.loss : nullptr);
  return hipGetLastError();
}
}  // namespace

int64_t distill_loss_workspace_bytes(int B) { return (int64_t)sizeof(double) * kDistillSums * loss_blocks(B); }
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
