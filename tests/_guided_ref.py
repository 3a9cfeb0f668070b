"""The guided loss of include/bbvec.h ("search-guided PPO") restated in numpy fp64, shared by
tests/test_guided_cpu.py and the GPU tests.  It calls none of the code under test.

  total = policy_coef * policy_loss + value_coef * value_loss - entropy_coef * entropy + distill_coef * cross_entropy

The distillation half is tests/_distill_ref.reference.  The PPO half is written out here, per row with M the set
mask bits (a row with empty M adds nothing and has no gradient):
  p = softmax of the logits over M (0 outside);  P = p / sum p;  logp = log(clamp(P[a], eps, 1 - eps)), eps = f32 eps
  entropy = -sum_M n log(max(n, 1e-10)),  n = p / max(sum_M p, 1e-10)
  ratio = exp(logp - old_logp);  policy = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A);  value = (v - ret)^2
  approx_kl = (ratio - 1) - log(ratio);  clipped = |ratio - 1| > clip
Gradient rules, spelled out (autograd's): min passes its gradient to the smaller argument and splits a tie half and
half; clamp passes it on the closed interval [lo, hi]; log(clamp(x)) divides by the clamped value.  The gradient
below is derived by hand from those rules; test_guided_cpu.py checks it against central finite differences of
``forward``.
"""
import numpy as np

import _distill_ref as D

EPS32 = float(np.finfo(np.float32).eps)
STATS = ("policy_loss", "value_loss", "entropy", "total_loss", "approx_kl", "clip_fraction",
         "cross_entropy", "kl", "target_entropy", "policy_entropy", "agreement", "rows")

# what the tests call with: the clip range, PPO's coefficients, a distillation coefficient, and the corners
# (policy, value, entropy, distill): PPO alone, distillation that fits the critic, PPO regularised to the teacher
CLIP = 0.2
VC, EC, BETA = 0.5, 0.01, 0.3
CORNERS = {"ppo": (1.0, VC, EC, 0.0), "distill+critic": (0.0, VC, 0.0, 1.0), "guided": (1.0, VC, EC, BETA)}


def check_stats(got, want, B):
    """got, want: 12 statistics (STATS) as float64 arrays, at the tolerances of the issue: rtol 1e-5 / atol 1e-6,
    clip_fraction within 2 / B, agreement (a count over B) and rows exact."""
    smooth = [0, 1, 2, 3, 4, 6, 7, 8, 9]
    np.testing.assert_allclose(got[smooth], want[smooth], rtol=1e-5, atol=1e-6)
    assert abs(got[5] - want[5]) <= 2.0 / B
    assert round(got[10] * B) == round(want[10] * B) and abs(got[10] - want[10]) < 1e-6
    assert got[11] == want[11]


def check_grads(dl, dv, want, mask_bits):
    """dvalues rtol 1e-5 / atol 1e-9, dlogits rtol 1e-4 / atol 1e-5 max|grad|; 0 outside M and in empty-M rows."""
    np.testing.assert_allclose(dv, want["dvalues"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(dl, want["dlogits"], rtol=1e-4, atol=1e-5 * max(np.abs(want["dlogits"]).max(), 1e-30))
    M = D.mask_bool(mask_bits)
    assert not dl[~M].any(), "gradient outside the mask"
    assert not dl[~want["live"]].any() and not dv[~want["live"]].any(), "gradient in a row with empty M"


def _row(x, m, a):
    """The PPO half's forward quantities of one row with non-empty mask m (fp64)."""
    p = np.zeros(192)
    e = np.exp(x[m] - x[m].max())
    p[m] = e / e.sum()
    s = p.sum()
    Pa = p[a] / s
    c = min(max(Pa, EPS32), 1.0 - EPS32)
    ms_raw = p[m].sum()
    ms = max(ms_raw, 1e-10)
    n = np.where(m, p, 0.0) / ms
    ent = -(n[m] * np.log(np.maximum(n[m], 1e-10))).sum()
    return dict(p=p, s=s, Pa=Pa, c=c, logp=np.log(c), ms_raw=ms_raw, ms=ms, n=n, ent=ent)


def log_probs(logits, mask_bits, actions):
    """logp per row as the loss computes it (0 for an empty-M row): what the row generator centres old_logp on."""
    x = np.asarray(logits, np.float64)
    M = D.mask_bool(mask_bits)
    return np.array([_row(x[i], M[i], int(actions[i]))["logp"] if M[i].any() else 0.0 for i in range(x.shape[0])])


def forward(logits, values, mask_bits, actions, old_logp, adv, ret, q, clip, coefs):
    """The 12 statistics (STATS) in fp64; ``coefs`` = (policy, value, entropy, distill, tau); q may be None."""
    pc, vc, ec, dc, tau = (float(c) for c in coefs)
    x, v = np.asarray(logits, np.float64), np.asarray(values, np.float64).reshape(-1)
    B = x.shape[0]
    M = D.mask_bool(mask_bits)
    sums = np.zeros(5)
    for i in range(B):
        if not M[i].any():
            continue
        r = _row(x[i], M[i], int(actions[i]))
        ratio = np.exp(r["logp"] - float(old_logp[i]))
        A = float(adv[i])
        s1, s2 = ratio * A, min(max(ratio, 1.0 - clip), 1.0 + clip) * A
        sums += (-min(s1, s2), (v[i] - float(ret[i])) ** 2, r["ent"], (ratio - 1.0) - np.log(ratio),
                 float(abs(ratio - 1.0) > clip))
    pol, vl, ent, kl, cf = sums / B
    d = D.reference(x, mask_bits, q, tau)["stats"] if q is not None else np.zeros(6)
    total = pc * pol + vc * vl - ec * ent + dc * d[0]
    return np.array([pol, vl, ent, total, kl, cf, *d])


def reference(logits, values, mask_bits, actions, old_logp, adv, ret, q, clip, coefs, grad_loss=1.0):
    """Returns {"stats": f64 [12], "loss": f64, "dlogits": f64 [B, 192], "dvalues": f64 [B], "live": bool [B]}:
    the gradients of grad_loss * total_loss."""
    pc, vc, ec, dc, tau = (float(c) for c in coefs)
    x, v = np.asarray(logits, np.float64), np.asarray(values, np.float64).reshape(-1)
    B = x.shape[0]
    g = float(grad_loss)
    M = D.mask_bool(mask_bits)
    stats = forward(logits, values, mask_bits, actions, old_logp, adv, ret, q, clip, coefs)
    dl = np.zeros((B, 192))
    dv = np.zeros(B)
    for i in range(B):
        m = M[i]
        if not m.any():
            continue
        a, A = int(actions[i]), float(adv[i])
        r = _row(x[i], m, a)
        p = r["p"]
        ratio = np.exp(r["logp"] - float(old_logp[i]))
        inside = 1.0 - clip <= ratio <= 1.0 + clip
        s1, s2 = ratio * A, min(max(ratio, 1.0 - clip), 1.0 + clip) * A
        w1, w2 = (1.0, 0.0) if s1 < s2 else ((0.0, 1.0) if s2 < s1 else (0.5, 0.5))  # d min / d (s1, s2)
        dpol_dratio = -(w1 * A + w2 * (A if inside else 0.0))
        dpol_dPa = dpol_dratio * ratio * ((1.0 / r["c"]) if EPS32 <= r["Pa"] <= 1.0 - EPS32 else 0.0)
        # d row / d p: the policy term through P_a = p_a / s, the entropy through n = p / ms on M
        grow = np.full(192, -pc * dpol_dPa * p[a] / r["s"] ** 2)
        grow[a] += pc * dpol_dPa / r["s"]
        dent_dn = np.where(m, -(np.log(np.maximum(r["n"], 1e-10)) + (r["n"] >= 1e-10)), 0.0)
        dent_dp = dent_dn / r["ms"]
        if r["ms_raw"] >= 1e-10:
            dent_dp = dent_dp - np.where(m, (dent_dn * p).sum() / r["ms"] ** 2, 0.0)
        grow += -ec * np.where(m, dent_dp, 0.0)
        dl[i] = g / B * p * (grow - (grow * p).sum())  # the softmax over M: p = 0 outside
        dv[i] = g / B * vc * 2.0 * (v[i] - float(ret[i]))
    if q is not None:
        dl += D.reference(x, mask_bits, q, tau, grad_loss=g * dc)["dlogits"]
    return {"stats": stats, "loss": stats[3], "dlogits": dl, "dvalues": dv, "live": M.any(axis=1)}


def synthetic(B, seed, density="mixed", kinds=True):
    """Seeded rows on ``_distill_ref.synthetic`` (its row kinds and densities): (logits f32 [B, 192], values f32 [B],
    mask words int64 [B, 3], actions int64 [B] inside M (0 for an empty M), old_logp f32 [B], adv f32 [B], ret f32
    [B], q int64 [B, 192]).  old_logp puts the ratio, cycling by row, at exactly 1 (the row's own log-prob), inside
    the clip range of 0.2 ([0.85, 1.15]) and outside it on either side ([0.5, 0.75], [1.25, 1.6]): away from the
    clip boundaries, where the gradient jumps.  Every fourth advantage is 0; rows with one legal action come with
    the "one" and "mixed" densities."""
    logits, mb, q = D.synthetic(B, seed, density=density, kinds=kinds)
    rng = np.random.default_rng(seed + 77)
    M = D.mask_bool(mb)
    actions = np.array([rng.choice(np.flatnonzero(M[i])) if M[i].any() else 0 for i in range(B)], np.int64)
    values = rng.standard_normal(B).astype(np.float32)
    ret = (values + rng.standard_normal(B) * 0.7).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    adv[3::4] = 0.0
    r = np.ones(B)
    for i in range(B):
        k = (i + seed) % 4
        r[i] = (1.0, rng.uniform(0.85, 1.15), rng.uniform(0.5, 0.75), rng.uniform(1.25, 1.6))[k]
    old = (log_probs(logits, mb, actions) - np.log(r)).astype(np.float32)
    return logits, values, mb, actions, old, adv, ret, q
