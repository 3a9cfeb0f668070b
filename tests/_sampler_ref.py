"""The masked policy head of csrc/bb_ppo.hip's masked_sample_kernel restated in numpy fp64, and the named corner rows
that tests/test_sampler_cpu.py and tests/test_gpu_sampler_edges.py feed it.  It calls none of the code under test.

Per row, from the f32 logits as given and a bool mask M (network.py:173-180, 210-262):
  p    = softmax of the logits over M (0 elsewhere)
  P    = p / sum p                                            Categorical(probs=p) normalises again
  logp = log(clamp(P[a], eps32, 1 - eps32))                   Categorical.log_prob (clamp_probs)
  ent  = -sum_M qn log(clamp(qn, 1e-10)), qn = p / clamp(sum_M p, 1e-10)
The clamp constants are the f32 values (eps32 = 2^-23, float32(1) - eps32, float32(1e-10)), widened.

A row with an empty M has no distribution (every quantity is NaN by construction): ``reference`` refuses one.
"""
import numpy as np

from _distill_ref import mask_words  # bool [B, 192] -> int64 [B, 3], the layout of include/bbvec.h

EPS32 = float(np.finfo(np.float32).eps)
ONE_M_EPS32 = float(np.float32(1.0) - np.finfo(np.float32).eps)
TINY32 = float(np.float32(1e-10))

# the project's fp32 tolerance (north_star; tests/test_gpu_ppo_kernels.py) for log-prob and entropy.  Derivable: the
# kernel's P is within 4 ulp of exact (K_ULP's comment there), so log P moves by <= 4 * 2^-24 = 2.4e-7, plus one logf
# rounding on |logp| <= 16 (log eps32 = -15.94; 1 ulp = 9.5e-7); the entropy is <= 192 terms |q log q| <= 1/e, each
# with a relative error of a few 2^-24, summed in fp32: well under 192 * 0.37 * 1e-6 / (1 + 5.26) of the bound.
RTOL = ATOL = 1e-5

U_EDGES = tuple(np.float32(v) for v in (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0))
U_THIRD = np.float32(1.0 / 3.0)  # on `equal`: the CDF boundary after action 63, K_ULP's rule decides
SINGLE_AT = (0, 63, 64, 127, 128, 191)  # both edges of every 64-bit mask word
EQUAL_VALUES = (0.0, 3e38, -3e38)
LEAD0_AT, TRAIL0_AT, TRAIL0_LAST = 150, 10, 179
TIE2_AT = (70, 130)


def reference(logits, mask, action):
    """logits f32 [B, 192], mask bool [B, 192] with a legal action in every row, action int [B] ->
    (P f64 [B, 192], logp f64 [B], entropy f64 [B])."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    m = np.asarray(mask, bool)
    a = np.asarray(action, np.int64)
    assert m.any(axis=1).all(), "a row without a legal action has no reference"
    B = x.shape[0]
    mx = np.where(m, x, -np.inf).max(axis=1, keepdims=True)
    e = np.where(m, np.exp(np.where(m, x - mx, 0.0)), 0.0)
    p = e / e.sum(axis=1, keepdims=True)
    P = p / p.sum(axis=1, keepdims=True)
    logp = np.log(np.clip(P[np.arange(B), a], EPS32, ONE_M_EPS32))
    mp = np.where(m, p, 0.0)
    qn = mp / np.maximum(mp.sum(axis=1, keepdims=True), TINY32)
    ent = -np.where(m, qn * np.log(np.maximum(qn, TINY32)), 0.0).sum(axis=1)
    return P, logp, ent


def _random_mask(rng, density):
    m = rng.random(192) < density
    m[rng.integers(0, 192)] = True
    return m


def _kinds():
    """[(kind, logits f32 [192], mask bool [192])], in a fixed order."""
    rng = np.random.default_rng(20240)
    out = []
    for k in SINGLE_AT:
        m = np.zeros(192, bool)
        m[k] = True
        out.append((f"single@{k}", rng.standard_normal(192) * 3.0, m))
    for v in EQUAL_VALUES:
        out.append((f"equal:{v:g}", np.full(192, v), np.ones(192, bool)))
    x = rng.standard_normal(192)
    m = _random_mask(rng, 0.3)
    m[list(TIE2_AT)] = True
    x[list(TIE2_AT)] = np.float32(x[m].max() + 1.5)  # two equal maxima, in words 1 and 2
    out.append(("tie2", x, m))
    x = rng.standard_normal(192) * 1e4
    m = _random_mask(rng, 0.5)
    m[191] = True
    x[191] = -2e4  # the last legal action is never the maximum
    out.append(("spread", x, m))
    x = np.full(192, -200.0)
    x[LEAD0_AT] = 0.0
    out.append(("lead0", x, np.ones(192, bool)))
    x = np.full(192, -200.0)
    x[TRAIL0_AT] = 0.0
    out.append(("trail0", x, np.arange(192) <= TRAIL0_LAST))
    for dname, dens in (("one", 0.0), ("tenth", 0.1), ("all", 1.0)):
        for scale in (1.0, 30.0):
            out.append((f"random:{dname}:{scale:g}", rng.standard_normal(192) * scale, _random_mask(rng, dens)))
    out.append(("empty", rng.standard_normal(192), np.zeros(192, bool)))
    return [(k, np.asarray(x, np.float32), m) for k, x, m in out]


def corner_rows():
    """Every kind at every uniform of U_EDGES (`equal` also at 1/3), kind-major ->
    {"kind": [R] str, "logits": f32 [R, 192], "mask": bool [R, 192], "u": f32 [R], "empty": bool [R]}."""
    kind, logits, mask, u = [], [], [], []
    for k, x, m in _kinds():
        for uv in U_EDGES + ((U_THIRD,) if k.startswith("equal") else ()):
            kind.append(k)
            logits.append(x)
            mask.append(m)
            u.append(uv)
    mask = np.stack(mask)
    return {"kind": np.array(kind), "logits": np.stack(logits), "mask": mask, "u": np.array(u, np.float32),
            "empty": ~mask.any(axis=1)}


# (n, first corner row): n rows from there on, cycling.  1: trail0 at u = 1 alone (the fallback in a one-row launch);
# 2 .. 5: the empty row with a neighbour on either side where n allows, and the word-edge single rows; 63, 64, 65: the
# blocks-of-4-rows boundary at three phases of the catalogue; 257 covers every row more than twice.
def batches(rows):
    R = len(rows["kind"])
    first = {k: int(np.flatnonzero(rows["kind"] == k)[0]) for k in set(rows["kind"].tolist())}
    return [(1, first["trail0"] + 4), (2, first["empty"] - 1), (3, first["empty"] + 3), (4, first["single@63"] + 3),
            (5, first["lead0"]), (63, 0), (64, 40 % R), (65, 80 % R), (257, 11)]


def take(rows, n, start):
    """The batch (n, start) of ``batches``: {"idx": corner row of each batch row, ...the rows' fields}."""
    idx = (start + np.arange(n)) % len(rows["kind"])
    return {"idx": idx, **{k: v[idx] for k, v in rows.items()}}


def big_rows(n, seed=65536):
    """n rows, no two equal: row i's mask density and logit scale cycle with i, and its forced legal action is
    (37 i) % 192.  -> (logits f32 [n, 192], mask bool [n, 192])."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    scale = np.array([0.5, 1.0, 3.0, 10.0, 30.0], np.float32)[i % 5]
    logits = rng.standard_normal((n, 192), dtype=np.float32) * scale[:, None]
    dens = np.array([0.02, 0.1, 0.3, 0.6, 0.9, 1.0, 0.05])[i % 7]
    mask = rng.random((n, 192), dtype=np.float32) < dens[:, None]
    mask[i, (37 * i) % 192] = True
    return logits, mask


def errors(lp, ent, logits, mask, action):
    """Worst |error| / (ATOL + RTOL |ref|) of log-prob and entropy against ``reference`` at ``action`` (<= 1 passes),
    and the worst absolute errors -> (lp_ratio, ent_ratio, lp_abs, ent_abs)."""
    _, lp64, ent64 = reference(logits, mask, action)
    dl, de = np.abs(np.asarray(lp, np.float64) - lp64), np.abs(np.asarray(ent, np.float64) - ent64)
    return (float((dl / (ATOL + RTOL * np.abs(lp64))).max()), float((de / (ATOL + RTOL * np.abs(ent64))).max()),
            float(dl.max()), float(de.max()))


__all__ = ["reference", "corner_rows", "batches", "take", "big_rows", "errors", "mask_words"]
