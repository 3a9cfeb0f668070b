// bb_loss_rows.h -- the row arithmetic of the masked policy head (gfx950), once: what masked_sample_kernel
// (bb_ppo.hip) and the three fused loss kernels (bb_loss.hip, bb_distill.hip, bb_guided.hip) compute per row.
//
// One wave per row, 3 entries per lane (action j * 64 + lane); m[j]: the action is in the mask M.  fp32 with
// torch's operation order, explicit round-to-nearest operations.
//   masked_softmax  mx = max of the logits over M, e = exp(x - mx) on M (0 elsewhere), se = sum e
//   categorical     p = e / se; Categorical(probs) normalises again: P = p / sum p
//   cat_logp        log(clamp(P[a], eps, 1 - eps))                        Categorical.log_prob (clamp_probs)
//   masked_entropy  -sum_M qn log(clamp(qn, 1e-10)), qn = p / clamp(sum_M p, 1e-10)   (network.py:232-262)
//   ppo_row         ratio = exp(logp - old_logp), pol = -min(ratio A, clamp(ratio, 1 - c, 1 + c) A),
//                   (v - ret)^2, approx_kl = (r - 1) - log r, clipped = |r - 1| > c; backward by autograd's rules:
//                   torch.min splits ties half/half, clamp passes the gradient on its closed interval, log divides
//                   by the clamped value
//   distill_row     S = the a in M with q[a] != INT64_MIN, qmax = max q over S; t = softmax over S of
//                   float(q - qmax) / tau (the difference in int64, exact; below -2^31: 0), or with tau == 0 the
//                   one-hot of the lowest a attaining qmax; logpi = (x - mx) - log(se), pi = exp(logpi);
//                   ce = -sum_{t > 0} t logpi, ht = -sum_{t > 0} t log t, hp = -sum_M pi logpi,
//                   agree = [lowest argmax of the logits over M == lowest argmax of q over S]; gradient pi - t
// Logits, values and their gradients are f32 or bf16 (BF): widened exactly on load, rounded to nearest even on
// store -- the values of autograd's casts around an fp32 loss, without the cast kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>
#include <stdint.h>

namespace bb {

constexpr int kLossThreads = 256;                  // the loss kernels' block: one row per wave
constexpr int kLossRows = kLossThreads / 64;       // rows (waves) per block
constexpr float kEps32 = 1.1920928955078125e-07f;  // torch.finfo(float32).eps (clamp_probs)

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int64_t wave_max64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t u = (int64_t)__shfl_xor((long long)v, o);
    v = u > v ? u : v;
  }
  return v;
}
// the three ballots of a per-entry predicate (word j = actions j * 64 ...)
struct Ballot3 {
  uint64_t b[3];
  __device__ __forceinline__ bool any() const { return (b[0] | b[1] | b[2]) != 0ull; }
  // the lowest action whose bit is set, -1 if none
  __device__ __forceinline__ int lowest() const {
    if (b[0]) return __builtin_ctzll(b[0]);
    if (b[1]) return 64 + __builtin_ctzll(b[1]);
    if (b[2]) return 128 + __builtin_ctzll(b[2]);
    return -1;
  }
};
__device__ __forceinline__ Ballot3 ballot3(bool p0, bool p1, bool p2) {
  return Ballot3{{__ballot(p0), __ballot(p1), __ballot(p2)}};
}

template <bool BF>
__device__ __forceinline__ float ld(const void* __restrict__ p, int64_t i) {
  if constexpr (BF) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
  return reinterpret_cast<const float*>(p)[i];
}
template <bool BF>
__device__ __forceinline__ void st(void* __restrict__ p, int64_t i, float v) {
  if constexpr (BF) {
    const __hip_bfloat16 b = __float2bfloat16(v);  // round to nearest even, as torch's cast
    reinterpret_cast<uint16_t*>(p)[i] = *reinterpret_cast<const uint16_t*>(&b);
  } else {
    reinterpret_cast<float*>(p)[i] = v;
  }
}
// a row's 3 entries per lane
template <bool BF>
__device__ __forceinline__ void st_row(void* __restrict__ p, int64_t row, int lane, const float (&v)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) st<BF>(p, row * 192 + j * 64 + lane, v[j]);
}

struct Softmax {
  float mx, e[3], se;
};
__device__ __forceinline__ Softmax masked_softmax(const float (&x)[3], const bool (&m)[3]) {
  Softmax r;
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (m[j]) mx = fmaxf(mx, x[j]);
  r.mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r.e[j] = m[j] ? expf(__fsub_rn(x[j], r.mx)) : 0.f;
    se = __fadd_rn(se, r.e[j]);
  }
  r.se = wave_sum(se);
  return r;
}

// Categorical(probs = p): p and its sum sp (P = p / sp)
struct Cat {
  float p[3], sp;
};
__device__ __forceinline__ Cat categorical(const Softmax& s) {
  Cat c;
  float s0 = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    c.p[j] = __fdiv_rn(s.e[j], s.se);
    s0 = __fadd_rn(s0, c.p[j]);
  }
  c.sp = wave_sum(s0);
  return c;
}
// log_prob of action a: p[a], P[a] and log(clamp(P[a], eps, 1 - eps)), in all lanes
struct CatLogp {
  float p_a, pa, logp;
};
__device__ __forceinline__ CatLogp cat_logp(const Cat& c, int64_t a) {
  const int aj = (int)(a >> 6), al = (int)(a & 63);
  CatLogp r;
  r.p_a = __shfl(aj == 0 ? c.p[0] : (aj == 1 ? c.p[1] : c.p[2]), al);
  r.pa = __fdiv_rn(r.p_a, c.sp);
  r.logp = logf(fminf(fmaxf(r.pa, kEps32), 1.f - kEps32));
  return r;
}
struct Entropy {
  float ms_raw, ms;    // sum of p over M, and clamped at 1e-10
  float qn[3], lq[3];  // masked p / ms and its clamped logarithm
  float ent;
};
__device__ __forceinline__ Entropy masked_entropy(const Cat& c, const bool (&m)[3]) {
  Entropy r;
  float ms = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) ms = __fadd_rn(ms, m[j] ? c.p[j] : 0.f);
  r.ms_raw = wave_sum(ms);
  r.ms = fmaxf(r.ms_raw, 1e-10f);
  float h = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r.qn[j] = __fdiv_rn(m[j] ? c.p[j] : 0.f, r.ms);
    r.lq[j] = logf(fmaxf(r.qn[j], 1e-10f));
    h = __fadd_rn(h, m[j] ? __fmul_rn(r.qn[j], r.lq[j]) : 0.f);
  }
  r.ent = -wave_sum(h);
  return r;
}

// The per-row inputs of the PPO loss, and what scales its terms: clip, the policy / value / entropy coefficients,
// and for GRAD the loss gradient g and 1 / B.
struct PpoRowIn {
  int64_t a;
  float old_logp, adv, ret, value;
};
struct PpoScale {
  float clip, pcoef, vcoef, ecoef, g, invB;
};
// STATS: adds the row's pol, vloss, ent, kl, clipped to acc[0..4].  GRAD: dvalue, and dz[j] = d loss / d logit of
// the row's entries (p (gp - sum gp p): an entry outside M has p = 0).
template <bool STATS, bool GRAD>
__device__ __forceinline__ void ppo_row(const Softmax& sm, const bool (&m)[3], const PpoRowIn& in, const PpoScale& k,
                                        int lane, double* acc, float& dvalue, float (&dz)[3]) {
  const Cat c = categorical(sm);
  const CatLogp lp = cat_logp(c, in.a);
  const Entropy en = masked_entropy(c, m);
  const float A = in.adv, clip = k.clip;
  const float ratio = expf(__fsub_rn(lp.logp, in.old_logp));
  const float s1 = __fmul_rn(ratio, A), s2 = __fmul_rn(fminf(fmaxf(ratio, 1.f - clip), 1.f + clip), A);
  const float dv = __fsub_rn(in.value, in.ret);
  if (STATS) {
    const float rm1 = __fsub_rn(ratio, 1.f);
    acc[0] += (double)(-fminf(s1, s2));
    acc[1] += (double)__fmul_rn(dv, dv);
    acc[2] += (double)en.ent;
    acc[3] += (double)__fsub_rn(rm1, logf(ratio));
    acc[4] += fabsf(rm1) > clip ? 1.0 : 0.0;
  }
  if (GRAD) {
    // d loss / d min(s1, s2) = -g policy_coef / B; torch.min splits ties half/half
    const float gmin = -(k.g * k.pcoef) * k.invB;
    const float g1 = s1 < s2 ? gmin : (s1 > s2 ? 0.f : 0.5f * gmin);
    const float g2 = s2 < s1 ? gmin : (s2 > s1 ? 0.f : 0.5f * gmin);
    const bool in_clip = ratio >= 1.f - clip && ratio <= 1.f + clip;
    const float glogp = (g1 * A + (in_clip ? g2 * A : 0.f)) * ratio;  // d exp(x)/dx = exp(x)
    dvalue = k.vcoef * k.g * k.invB * 2.f * dv;                       // mse
    const float gent = -k.ecoef * k.g * k.invB;                       // entropy_coef * (-mean(ent))
    // log(clamp(P_a, eps, 1 - eps)): passes where eps <= P_a <= 1 - eps, divided by the clamped value
    const float gPa = (lp.pa >= kEps32 && lp.pa <= 1.f - kEps32) ? glogp / lp.pa : 0.f;
    // P = p / s: gp_k = [k == a] gPa / s - gPa p_a / s^2
    const int aj = (int)(in.a >> 6), al = (int)(in.a & 63);
    const float corr = gPa * lp.p_a / (c.sp * c.sp);
    // entropy = -sum m q log(clamp(q, 1e-10)), q = m p / clamp(ms, 1e-10):
    //   d/dq_j = -m_j (log(clamp(q_j)) + [q_j >= 1e-10])
    float gq[3], sgqm = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gq[j] = m[j] ? -gent * (en.lq[j] + (en.qn[j] >= 1e-10f ? 1.f : 0.f)) : 0.f;
      sgqm += m[j] ? gq[j] * c.p[j] : 0.f;
    }
    sgqm = wave_sum(sgqm);
    const float gms = en.ms_raw >= 1e-10f ? -sgqm / (en.ms * en.ms) : 0.f;
    float gp[3], dot = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gp[j] = ((j == aj && lane == al) ? gPa / c.sp : 0.f) - corr;
      if (m[j]) gp[j] += gq[j] / en.ms + gms;
      dot += gp[j] * c.p[j];
    }
    dot = wave_sum(dot);
    // softmax backward: dz_k = p_k (gp_k - sum_j gp_j p_j)
#pragma unroll
    for (int j = 0; j < 3; ++j) dz[j] = c.p[j] * (gp[j] - dot);
  }
}

// A row with non-empty S (s[j] = m[j] && qv[j] != INT64_MIN; the caller decides what an empty S means), on the
// masked softmax it is given (mx, se).  STATS: adds ce, ht, hp, agree and 1 (the row) to acc[0..4].  GRAD:
// dg[j] = scale (pi - t) on M, 0 elsewhere; scale = the loss gradient times the distillation coefficient, / B.
template <bool STATS, bool GRAD>
__device__ __forceinline__ void distill_row(const float (&x)[3], const bool (&m)[3], const bool (&s)[3],
                                            const int64_t (&qv)[3], float mx, float se, float tau, float scale,
                                            int lane, double* acc, float (&dg)[3]) {
  const float lse = logf(se);
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
  qm = wave_max64(qm);
  const int qarg = ballot3(s[0] && qv[0] == qm, s[1] && qv[1] == qm, s[2] && qv[2] == qm).lowest();
  float t[3];
  if (tau > 0.f) {
    float wt[3], z = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t d = s[j] ? qv[j] - qm : 0;  // <= 0, exact
      wt[j] = (s[j] && d >= -2147483648ll) ? expf(__fdiv_rn((float)d, tau)) : 0.f;
      z = __fadd_rn(z, wt[j]);
    }
    z = wave_sum(z);  // >= 1: the maximum's weight is 1
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
    ce = wave_sum(ce);
    ht = wave_sum(ht);
    hp = wave_sum(hp);
    const int parg = ballot3(m[0] && x[0] == mx, m[1] && x[1] == mx, m[2] && x[2] == mx).lowest();
    acc[0] += (double)-ce;
    acc[1] += (double)-ht;
    acc[2] += (double)-hp;
    acc[3] += parg == qarg ? 1.0 : 0.0;
    acc[4] += 1.0;
  }
  if (GRAD) {
#pragma unroll
    for (int j = 0; j < 3; ++j) dg[j] = m[j] ? __fmul_rn(scale, __fsub_rn(pi[j], t[j])) : 0.f;
  }
}

inline int loss_blocks(int B) {
  const int b = (B + kLossRows - 1) / kLossRows;
  return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

}  // namespace bb
