"""The optimizer step, the weight casts and the dropout mask of csrc/bb_optim.hip restated in numpy (fp64 and integer
arithmetic), and the catalogue of cases tests/test_gpu_adam_edges.py runs.  It calls none of the code under test.

adam_clip_ref       nn.utils.clip_grad_norm_ + torch.optim.Adam (weight decay 0) in float64; with ``norm32`` (the fp32
                    norm an implementation reported) it replays the kernel's documented roundings instead (the header of
                    bb_optim.hip and adam_elem): the clip coefficient in fp32 from that norm, g' one fp32 product, the
                    moments in fp64 from the fp32 operands rounded once, the bias corrections rounded to fp32.
bf16_rne            f32 -> bf16, round to nearest even, on the bit patterns.
dropout_ref         the keep mask of bb_dropout_forward: Philox4x32-10, counter (element / 4, offset), key seed.
cast_patterns       the fp32 bit patterns the cast tests run.
adam_cases / build  the Adam catalogue: views into flat guarded buffers.
"""
from collections import namedtuple

import numpy as np

from oracle.philox import philox4x32_10

LR, EPS, BETA1, BETA2 = 3e-4, 1e-5, 0.9, 0.999  # the agent's optimizer (agents/ppo.py)
CHUNK = 2048  # BB_ADAM_CHUNK
GUARD_SQ = 1e16  # the finaliser's guard on a chunk's sum of squares
MAX_TENSORS = 48  # BB_OPT_MAX_TENSORS
GUARD = 4  # guard floats between neighbouring views and at both ends (at least)
SENTINEL = np.float32(-6.2578e28)
F32_TINY = float(np.finfo(np.float32).tiny)
F32_MAX = float(np.finfo(np.float32).max)

f32, f64 = np.float32, np.float64


def adam_clip_ref(p, g, m, v, step, lr, b1, b2, eps, max_norm, norm32=None):
    """Lists of arrays (one per tensor) and of prior step counts -> dict of norm64, coef, and lists g, m, v, p (the
    new values, float64 arrays), step (prior + 1) and upd64 = p - p'."""
    g64 = [np.asarray(x, f64) for x in g]
    norm64 = float(np.sqrt(sum(float((x * x).sum()) for x in g64)))
    exact = norm32 is None
    if exact:
        coef = min(max_norm / (norm64 + 1e-6), 1.0)
    else:
        coef = min(f32(max_norm) / (f32(norm32) + f32(1e-6)), f32(1.0))
        assert type(coef) is np.float32
    out = {"norm64": norm64, "coef": coef, "g": [], "m": [], "v": [], "p": [], "step": [], "upd64": []}
    for pt, gt, mt, vt, st in zip(p, g64, m, v, step):
        pt, mt, vt = np.asarray(pt, f64), np.asarray(mt, f64), np.asarray(vt, f64)
        st = float(st) + 1.0
        if exact:
            gn = gt * coef
            mn = b1 * mt + (1.0 - b1) * gn
            vn = b2 * vt + (1.0 - b2) * gn * gn
            bc1, bc2s = 1.0 - b1 ** st, np.sqrt(1.0 - b2 ** st)
        else:
            gn = (gt.astype(f32) * coef).astype(f64)  # one IEEE fp32 product
            mn = (b1 * mt + (1.0 - b1) * gn).astype(f32).astype(f64)
            vn = (b2 * vt + (1.0 - b2) * gn * gn).astype(f32).astype(f64)
            bc1, bc2s = f64(f32(1.0 - b1 ** st)), f64(f32(np.sqrt(1.0 - b2 ** st)))
        upd = (lr / bc1) * mn / (np.sqrt(vn) / bc2s + eps)
        out["g"].append(gn)
        out["m"].append(mn)
        out["v"].append(vn)
        out["p"].append(pt - upd)
        out["upd64"].append(upd)
        out["step"].append(st)
    return out


def bf16_rne(x_f32):
    """fp32 array -> uint16 bf16 patterns, round to nearest even on the bits; NaN stays NaN (quiet bit set)."""
    b = np.ascontiguousarray(x_f32, dtype=f32).view(np.uint32).astype(np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return np.where(nan, (b >> 16) | 0x40, r).astype(np.uint16)


def is_nan_bf16(h):
    return (np.asarray(h, np.uint16) & 0x7FFF) > 0x7F80


def dropout_ref(n, p, seed, offset):
    """(keep mask [n], scale) of bb_dropout_forward: element e is kept when word e & 3 of
    philox4x32_10(e >> 2, offset, seed) >= uint32(float64(float32(p)) * 2^32); scale = 1 / float32(1 - p)."""
    pf = f32(p)
    t = float(pf) * 4294967296.0
    thresh = np.uint32(0xFFFFFFFF if t >= 4294967295.0 else int(t))
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = np.stack(philox4x32_10(q, int(offset), int(seed)), axis=1).reshape(-1)[:n]
    scale = f32(1.0 / float(f32(1.0 - float(pf))))
    return words >= thresh, scale


def cast_patterns():
    """uint32 fp32 bit patterns: every bf16 pattern widened, each one fp32 ulp up and down, each plus half a bf16
    step (the ties, on even and odd bf16 mantissas alike), fp32 subnormals, the largest finite fp32 (it rounds to
    infinity), +-0, +-inf, quiet and signalling NaNs."""
    wide = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    extra = [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF, 0x007F8000,
             0x80000001, 0x80008000, 0x80018000, 0x807FFFFF,  # subnormals (and their ties)
             0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # the largest finite, the last tie below infinity
             0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
             0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0x7F80FFFF, 0x7FFFFFFF]
    return np.concatenate([wide, wide + np.uint32(1), wide - np.uint32(1), wide + np.uint32(0x8000),
                           np.array(extra, dtype=np.uint32)])


# ---------------------------------------------------------------------------------------------------------------
# The Adam catalogue
# ---------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 2047, 2048, 2049, 4096, 4097, 6143)
# float offsets (p, g, m, v) of a view from a 16-byte boundary.  g1..g3: only the gradient misaligned -- the norm
# kernel and the update kernel both take their scalar paths; m1: only exp_avg -- the norm stays on float4 loads and
# the update goes scalar
ALIGNS = {"aligned": (0, 0, 0, 0), "all1": (1, 1, 1, 1), "g1": (0, 1, 0, 0), "g2": (0, 2, 0, 0), "g3": (0, 3, 0, 0),
          "m1": (0, 0, 1, 0)}
STATES = ("zero@0", "random@9", "random@999", "random@99999")
GRADS = ("normal", "zero", "mixed", "single0.25", "single0.5")
CHUNK_TOTALS = (2047, 2048, 2049, 2048 + 256 + 1)

# sizes: n per tensor; aligns: an ALIGNS key per tensor; state: a STATES entry; grad: a GRADS entry
Case = namedtuple("Case", "name sizes aligns state grad max_norm seed")


def adam_cases():
    out = []

    def add(name, sizes, aligns, state="zero@0", grad="normal", max_norm=0.5):
        if isinstance(aligns, str):
            aligns = (aligns,) * len(sizes)
        out.append(Case(name, tuple(sizes), tuple(aligns), state, grad, max_norm, 7000 + len(out)))

    for a in ALIGNS:  # every size in every alignment variant
        add(f"sizes-{a}", SIZES, a)
    mixed_al = tuple(list(ALIGNS)[i % len(ALIGNS)] for i in range(MAX_TENSORS))
    # exactly 48 tensors, sizes and alignments mixed, the last with a partial last chunk
    add("table48", [SIZES[(3 * i) % len(SIZES)] for i in range(MAX_TENSORS - 1)] + [2 * CHUNK + 517], mixed_al,
        state="random@9")
    add("mixed-align", SIZES, mixed_al[:len(SIZES)], state="random@9")
    for k in CHUNK_TOTALS[:3]:  # the finaliser's 8-wide loop: i + 7 * 256 < nchunks
        add(f"chunks{k}", [CHUNK * k - 5], "aligned")
    add(f"chunks{CHUNK_TOTALS[3]}", [CHUNK * 2048, CHUNK * 256 + 1], "aligned")
    for s in STATES[1:]:
        add(f"state-{s}", (5, 2049, 4097), ("aligned", "g1", "m1"), state=s)
    add("grad-zero", (5, 2049), ("aligned", "all1"), state="random@9", grad="zero")
    add("grad-mixed", (2047, 2049, 2048), ("aligned", "g2", "aligned"), state="random@9", grad="mixed", max_norm=1e9)
    add("grad-single0.25", (1,), "aligned", grad="single0.25")  # coef == 1: g comes back bit-identical
    add("grad-single0.5", (1,), "aligned", grad="single0.5")  # coef just below 1
    add("max-norm-1e9", (5, 2049, 4097), ("aligned", "g3", "m1"), state="random@999", max_norm=1e9)
    return out


def layout(case):
    """Per buffer (p, g, m, v): the start of every view in its flat buffer, and the buffer's length.  A view starts
    at its float offset from a 16-byte boundary, at least GUARD floats after its neighbour's end."""
    starts, totals = [], []
    for b in range(4):
        cur, st = 0, []
        for n, a in zip(case.sizes, case.aligns):
            s = -(-(cur + GUARD) // 4) * 4 + ALIGNS[a][b]
            st.append(s)
            cur = s + n
        starts.append(st)
        totals.append(-(-(cur + GUARD) // 4) * 4)
    return starts, totals


def gradients(case, k):
    """Step k's gradients, one fp32 array per tensor (a new draw per step for the random kinds)."""
    rng = np.random.default_rng(case.seed * 10 + k)
    out = []
    for t, n in enumerate(case.sizes):
        if case.grad == "normal":
            g = rng.standard_normal(n) * (0.02, 1.0, 0.3)[k % 3]
            g[np.abs(g) < 1e-6] = 1e-6
        elif case.grad == "zero":
            g = np.zeros(n)
        elif case.grad == "mixed":  # magnitudes 1e-12, 1 and 1e6, one per tensor
            g = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * (1e-12, 1.0, 1e6)[t % 3]
        else:
            g = np.full(n, float(case.grad[len("single"):]))
        out.append(g.astype(f32))
    return out


def build(case):
    """The case's start: dict of flat fp32 buffers p, m, v (guards = SENTINEL), the views' starts and the buffers'
    lengths, and the prior step counts.  Gradients come from ``flat_gradients`` per step."""
    rng = np.random.default_rng(case.seed)
    starts, totals = layout(case)
    g0 = gradients(case, 0)
    step0 = float(case.state.split("@")[1])
    flat = {k: np.full(totals[i], SENTINEL, f32) for i, k in ((0, "p"), (2, "m"), (3, "v"))}
    for t, n in enumerate(case.sizes):
        p = rng.standard_normal(n) * 0.1
        if case.state == "zero@0" and case.grad != "zero":
            m, v = np.zeros(n), np.zeros(n)
        else:
            ref = np.abs(g0[t].astype(f64)) if case.grad not in ("zero",) else np.full(n, 1e-2)
            ref = np.maximum(ref * (1.0 if case.max_norm > 1e8 else 1e-2), 1e-15)  # about the clipped size
            # exp_avg opposite in sign to the gradient on half the elements
            sign = np.where(np.arange(n) % 2 == 0, -1.0, 1.0) * np.where(g0[t] < 0, -1.0, 1.0)
            m = sign * ref * rng.uniform(0.5, 2.0, n)
            # exp_avg_sq far above, far below and about g^2, in thirds
            v = ref * ref * np.choose(np.arange(n) % 3, [1e8, 1e-8, 1.0]) * rng.uniform(0.5, 2.0, n)
        for k, a in (("p", p), ("m", m), ("v", v)):
            s = starts["pgmv".index(k)][t]
            flat[k][s:s + n] = a.astype(f32)
    return {"flat": flat, "starts": starts, "totals": totals, "steps": [step0] * len(case.sizes)}


def flat_gradients(case, k, starts, totals):
    buf = np.full(totals[1], SENTINEL, f32)
    for s, g in zip(starts[1], gradients(case, k)):
        buf[s:s + g.size] = g
    return buf


def views(flat, starts, sizes):
    return [flat[s:s + n] for s, n in zip(starts, sizes)]


def guards_intact(flat, starts, sizes):
    """Every float of ``flat`` outside the views still holds SENTINEL (bitwise)."""
    inside = np.zeros(flat.size, bool)
    for s, n in zip(starts, sizes):
        inside[s:s + n] = True
    return bool((flat.view(np.uint32)[~inside] == SENTINEL.view(np.uint32)).all())


def chunk_total(case):
    return sum(-(-n // CHUNK) for n in case.sizes)


def check_fair(case, steps=3):
    """Three chained fp64 steps from the case's start: no g^2, m' or v' is subnormal or overflows in fp32 (zero is
    neither), and no chunk's sum of squares reaches the guard's 1e16."""
    b = build(case)
    st, sz = b["starts"], case.sizes
    p, m, v = (views(b["flat"][k].astype(f64), st["pgmv".index(k)], sz) for k in "pmv")
    steps_now = b["steps"]

    def fair(x):
        a = np.abs(x[x != 0])
        return a.size == 0 or (a.min() >= F32_TINY and a.max() <= F32_MAX)

    for k in range(steps):
        g = gradients(case, k)
        for gt in g:
            g2 = gt.astype(f64) ** 2
            assert fair(g2), (case.name, k, "g^2")
            pad = np.zeros(-(-g2.size // CHUNK) * CHUNK)
            pad[:g2.size] = g2
            assert pad.reshape(-1, CHUNK).sum(axis=1).max() < 0.5 * GUARD_SQ,(case.name, k, "chunk partial")
        r = adam_clip_ref(p, g, m, v, steps_now, LR, BETA1, BETA2, EPS, case.max_norm)
        for name in ("g", "m", "v"):
            for x in r[name]:
                assert fair(x), (case.name, k, name)
            if name == "g":
                assert all(fair(x * x) for x in r["g"]), (case.name, k, "g'^2")
        p, m, v, steps_now = r["p"], r["m"], r["v"], r["step"]


# ---------------------------------------------------------------------------------------------------------------
# The bounds of tests/test_gpu_adam_edges.py (derived in its docstring), each as |err| / allowed
# ---------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
NORM_ULPS, PARAM_UPD_ULPS, MOMENT_SHARE = 6.0, 8.0, 1e-4


def ordered(x_f32):
    """fp32 -> int64 that orders as the values do and steps by 1 per ulp (+0 and -0 both map to 0)."""
    b = np.ascontiguousarray(x_f32, dtype=f32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def measure(got, ref, coef_is_one, g_in):
    """got: fp32 arrays norm (scalar), and lists g, m, v, p as an implementation left them; ref: adam_clip_ref with
    that norm.  -> dict of the worst ratios to the bounds (<= 1 passes): norm, g_bits (0 or inf), m_ulp, v_ulp (worst
    ulp distance, bound 1), m_share, v_share (share of elements off the replay / 1e-4), p."""
    out = {"norm": abs(float(got["norm"]) - ref["norm64"]) / max(NORM_ULPS * U * ref["norm64"], 1e-300)
           if ref["norm64"] > 0 else (0.0 if float(got["norm"]) == 0.0 else np.inf)}
    total = sum(x.size for x in got["g"])
    same = all(np.array_equal(a.view(np.uint32), r.astype(f32).view(np.uint32)) for a, r in zip(got["g"], ref["g"]))
    if coef_is_one:
        same = same and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got["g"], g_in))
    out["g_bits"] = 0.0 if same else np.inf
    for k in ("m", "v"):
        d = [np.abs(ordered(a) - ordered(r.astype(f32))) for a, r in zip(got[k], ref[k])]
        out[k + "_ulp"] = float(max(x.max() for x in d))
        out[k + "_share"] = sum(int((x != 0).sum()) for x in d) / total / MOMENT_SHARE
    worst = 0.0
    for a, r, u in zip(got["p"], ref["p"], ref["upd64"]):
        allowed = PARAM_UPD_ULPS * U * np.abs(u) + U * np.abs(r)
        worst = max(worst, float((np.abs(a.astype(f64) - r) / np.maximum(allowed, 1e-300)).max()))
    out["p"] = worst
    return out
