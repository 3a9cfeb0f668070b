"""The distillation loss of include/bbvec.h ("policy distillation") restated in numpy fp64, shared by
tests/test_distill_cpu.py and tests/test_gpu_distill_loss.py.  It calls none of the code under test.

Per row: M = actions whose mask bit is set, S = the a in M with q[a] != INT64_MIN, qmax = max q over S.
Tie rules, spelled out: the argmax of q over S and the argmax of the logits over M are both the LOWEST action
index attaining the maximum (exact equality of int64 values, exact equality of the logits as given); at tau == 0 the
target is the one-hot of that lowest argmax of q.
"""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min
STATS = ("cross_entropy", "kl", "target_entropy", "policy_entropy", "agreement", "rows")


def mask_bool(mask_bits):
    """Mask words [B, 3] (int64 or uint64 bit patterns) -> bool [B, 192]: bit c of word p is action p * 64 + c."""
    w = np.ascontiguousarray(mask_bits).view(np.uint64).reshape(-1, 3)
    return ((w[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1, 192)


def mask_words(flags):
    """bool [B, 192] -> int64 [B, 3] words."""
    f = np.asarray(flags, bool).reshape(-1, 3, 64).astype(np.uint64)
    return (f << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).view(np.int64)


def lowest_argmax(values, where):
    """Per row the lowest index attaining the maximum of ``values`` over ``where`` (-1 for an empty row)."""
    out = np.full(values.shape[0], -1, np.int64)
    for i in range(values.shape[0]):
        idx = np.flatnonzero(where[i])
        if idx.size:
            best = idx[0]
            for a in idx[1:]:
                if values[i, a] > values[i, best]:  # strictly greater: ties stay with the lower index
                    best = a
            out[i] = best
    return out


def reference(logits, mask_bits, q, tau, grad_loss=1.0):
    """logits [B, 192] (any float dtype, taken as given), mask_bits [B, 3], q int64 [B, 192], tau >= 0.
    Returns {"stats": f64 [6], "loss": f64, "dlogits": f64 [B, 192], "t": f64 [B, 192], "qarg": [B], "parg": [B]}."""
    x = np.asarray(logits, np.float64)
    q = np.asarray(q, np.int64)
    B = x.shape[0]
    M = mask_bool(mask_bits)
    S = M & (q != INT64_MIN)
    has = S.any(axis=1)
    qarg, parg = lowest_argmax(q, S), lowest_argmax(x, M)
    t = np.zeros((B, 192))
    logpi = np.zeros((B, 192))
    pi = np.zeros((B, 192))
    dl = np.zeros((B, 192))
    ce = np.zeros(B)
    ht = np.zeros(B)
    hp = np.zeros(B)
    for i in np.flatnonzero(has):
        s, m = S[i], M[i]
        qmax = int(q[i, qarg[i]])
        if tau > 0:
            d = np.array([int(v) - qmax for v in q[i, s]], dtype=object)  # Python ints: exact
            w = np.array([np.exp(float(v) / float(tau)) if v >= -(2 ** 31) else 0.0 for v in d], np.float64)
            t[i, s] = w / w.sum()
        else:
            t[i, qarg[i]] = 1.0
        z = x[i, m] - x[i, m].max()
        logpi[i, m] = z - np.log(np.exp(z).sum())
        pi[i, m] = np.exp(logpi[i, m])
        pos = t[i] > 0
        ce[i] = -(t[i, pos] * logpi[i, pos]).sum()
        ht[i] = -(t[i, pos] * np.log(t[i, pos])).sum()
        pp = pi[i] > 0
        hp[i] = -(pi[i, pp] * logpi[i, pp]).sum()
        dl[i, m] = float(grad_loss) / B * (pi[i, m] - t[i, m])
    agree = ((qarg == parg) & has).astype(np.float64)
    stats = np.array([ce.sum() / B, (ce.sum() - ht.sum()) / B, ht.sum() / B, hp.sum() / B, agree.sum() / B,
                      float(has.sum())])
    return {"stats": stats, "loss": stats[0], "dlogits": dl, "t": t, "qarg": qarg, "parg": parg, "has": has}


def synthetic(B, seed, density="mixed", kinds=True):
    """Seeded rows: logits f32 [B, 192], mask words int64 [B, 3], q int64 [B, 192].  ``density``: "one" (1 legal
    action), "tenth" (~10% legal), "all" (192 legal) or "mixed" (cycling through the three).  With ``kinds`` the
    first rows are the special kinds, in this order as far as B allows: 0 empty M; 1 M non-empty and S empty; 2 an
    exact three-way tie at the maximum of q; 3 a row holding both 0 and -100000; 4 a difference beyond -2^31."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, 192)) * 2.0).astype(np.float32)
    q = rng.integers(-400, 400, (B, 192)).astype(np.int64)
    M = np.zeros((B, 192), bool)
    for i in range(B):
        kind = {"one": 0, "tenth": 1, "all": 2, "mixed": i % 3}[density]
        if kind == 0:
            M[i, rng.integers(192)] = True
        elif kind == 1:
            M[i] = rng.random(192) < 0.1
            M[i, rng.integers(192)] = True
        else:
            M[i] = True
    # illegal actions carry INT64_MIN, as bb_plan_values writes them; a few masked-out actions keep a value and a
    # few masked-in ones are INT64_MIN (a stale mask): S is then a proper subset of M
    q[~M & (rng.random((B, 192)) < 0.9)] = INT64_MIN
    stale = M & (rng.random((B, 192)) < 0.05)
    stale[np.arange(B), np.argmax(M, axis=1)] = False  # the first legal action keeps its value
    q[stale] = INT64_MIN
    if kinds:
        if B > 0:
            M[0] = False
        if B > 1:
            M[1] = False
            M[1, [3, 70, 191]] = True
            q[1] = INT64_MIN
        if B > 2:
            M[2] = True
            q[2] = rng.integers(-50, 50, 192)
            q[2, [17, 64, 130]] = 77
            logits[2, 64] = logits[2].max() + 1.0  # the policy's argmax is a tied action that is not the lowest
        if B > 3:
            M[3] = True
            q[3] = np.where(rng.random(192) < 0.5, 0, -100000)
            q[3, 5], q[3, 6] = 0, -100000
        if B > 4:
            M[4] = True
            q[4] = rng.integers(-100, 100, 192)
            q[4, 9] = -(2 ** 31) - 100 - 5   # below qmax - 2^31 whatever the maximum of the row
            q[4, 10] = -(2 ** 40)
            q[4, 11] = q[4].max() - 2 ** 31 + 200  # within 2^31 of the maximum: computed, underflows for small tau
    return logits, mask_words(M), q
