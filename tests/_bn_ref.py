"""Training-mode BatchNorm2d [+ ReLU] of include/bbvec.h (bb_bn_forward / bb_bn_backward) restated in numpy fp64, the
channel kinds that tests/test_gpu_batchnorm_edges.py mixes inside one tensor, and its bounds.  It calls none of the
code under test.

The input is the stored tensor (bf16 values widened exactly).  The statistics are those of x itself: ``pre_bias`` (a
preceding convolution's bias) shifts only the running mean.  With the ReLU the backward takes the mask it is given
(the fused forward's own y > 0: a tie at the kink may round either way).
"""
from collections import namedtuple

import numpy as np

KINDS = ("unit", "offset", "const", "tiny", "big", "dead")  # dead: only with the ReLU

Case = namedtuple("Case", "n c h nhwc bf16 relu pre_bias momentum shift")


def kinds_of(case):
    """The kind of every channel: the kinds in order from ``shift`` on, cycling (``dead`` only under the ReLU)."""
    names = KINDS if case.relu else KINDS[:-1]
    return np.array([names[(c + case.shift) % len(names)] for c in range(case.c)])


def fusable(c, h, nhwc, bf16):
    """bb_bn's shape rules (include/bbvec.h)."""
    esz = 2 if bf16 else 4
    if nhwc:
        return c * esz % 16 == 0 and 256 % (c * esz // 16) == 0
    return h * h * esz % 16 == 0 and h * h * esz <= 4096


def cases():
    """N in {1, 3, 33, 257} at 8x8 in both layouts, dtypes and ReLU settings, C cycling through what the layout and
    dtype allow (257 rows take the widest), pre_bias in every combination with the ReLU, momentum 0.1 and 0.25; then
    the other spatial sizes: NCHW f32 2x2, 4x4, 6x6 (9 vectors per row: 256 % 9 != 0), 16x16, 32x32 (256 vectors: the
    largest legal row), NCHW bf16 4x4, 16x16, 32x32, and NHWC at 6x6 and 2x2."""
    out = []
    for k, n in enumerate((1, 3, 33, 257)):
        for nhwc in (False, True):
            for bf16 in (False, True):
                cs = [c for c in (4, 8, 64, 128) if fusable(c, 8, nhwc, bf16)]
                for relu in (False, True):
                    out.append(Case(n, cs[-1] if n == 257 else cs[k % len(cs)], 8, nhwc, bf16, relu,
                                    (k + relu) % 2 == 0, 0.25 if k % 2 else 0.1, len(out)))
    for j, (n, c, h, nhwc, bf16) in enumerate([(33, 8, 2, False, False), (33, 4, 4, False, False),
                                                (33, 8, 6, False, False), (33, 64, 16, False, False),
                                                (5, 8, 32, False, False), (257, 8, 4, False, True),
                                                (33, 8, 16, False, True), (5, 4, 32, False, True),
                                                (33, 4, 6, True, False), (3, 8, 2, True, True)]):
        assert fusable(c, h, nhwc, bf16)
        out.append(Case(n, c, h, nhwc, bf16, j % 2 == 0, j % 3 == 0, 0.25 if j % 2 else 0.1, len(out)))
    return out


def case_id(k):
    return (f"N{k.n}-C{k.c}-{k.h}x{k.h}-{'nhwc' if k.nhwc else 'nchw'}-{'bf16' if k.bf16 else 'f32'}"
            f"{'-relu' if k.relu else ''}{'-pb' if k.pre_bias else ''}")


def inputs(case):
    """fp64 arrays of one case (the test casts x and dy to the case's dtype and takes what is stored):
    x, dy [N, C, H, W]; weight, bias, pre_bias (or None), running_mean, running_var [C]; kinds [C]."""
    rng = np.random.default_rng(1000 + case.shift)
    n, c, h = case.n, case.c, case.h
    kinds = kinds_of(case)
    z = rng.standard_normal((n, c, h, h))
    x = np.empty_like(z)
    weight = rng.random(c) + 0.5
    bias = rng.standard_normal(c) * 0.1
    for i, k in enumerate(kinds):
        if k == "offset":
            x[:, i] = 8.0 + 0.25 * z[:, i]
        elif k == "const":
            x[:, i] = 0.5
        elif k == "tiny":
            x[:, i] = 1e-3 * z[:, i]
        elif k == "big":
            x[:, i] = 1e3 * z[:, i]
        else:  # unit, dead
            x[:, i] = z[:, i]
        if k == "dead":
            weight[i], bias[i] = 0.01, -5.0
    return {"x": x, "dy": rng.standard_normal((n, c, h, h)), "weight": weight, "bias": bias,
            "pre_bias": 100.0 + 10.0 * rng.standard_normal(c) if case.pre_bias else None,
            "running_mean": 0.1 * rng.standard_normal(c), "running_var": rng.random(c) + 0.5, "kinds": kinds}


def reference(x, dy, weight, bias, pre_bias, running_mean, running_var, momentum, eps, relu, mask=None):
    """All fp64, x and dy [N, C, H, W] -> dict of y, mean, invstd, running_mean, running_var, dx, dweight, dbias,
    dpre_bias, and the sums of absolute terms behind dweight and dbias (abs_dweight, abs_dbias)."""
    ax = (0, 2, 3)
    sh = (1, -1, 1, 1)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(axis=ax)
    var = ((x - mean.reshape(sh)) ** 2).mean(axis=ax)
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean.reshape(sh)) * invstd.reshape(sh)
    y = xhat * weight.reshape(sh) + bias.reshape(sh)
    if relu:
        y = np.maximum(y, 0.0)
        g = dy * (mask if mask is not None else (y > 0))
    else:
        g = dy
    mu_u = mean + (pre_bias if pre_bias is not None else 0.0)
    out = {"y": y, "mean": mean, "invstd": invstd,
           "running_mean": (1.0 - momentum) * running_mean + momentum * mu_u,
           "running_var": (1.0 - momentum) * running_var + momentum * (var * M / (M - 1) if M > 1 else var)}
    out["dbias"] = g.sum(axis=ax)
    out["dweight"] = (g * xhat).sum(axis=ax)
    out["abs_dbias"] = np.abs(g).sum(axis=ax)
    out["abs_dweight"] = np.abs(g * xhat).sum(axis=ax)
    out["dx"] = (weight * invstd).reshape(sh) * (g - (out["dbias"] / M).reshape(sh)
                                                 - xhat * (out["dweight"] / M).reshape(sh))
    out["dpre_bias"] = out["dx"].sum(axis=ax)  # 0 but for rounding: the bias cancels in the output
    return out


# The bounds, each as |err| / allowed (<= 1 passes), the worst over the channels of one kind.
#   y, dx                       tests/test_gpu_ppo_kernels.py::test_fused_batchnorm_matches_torch's: rtol = tol,
#                               atol = tol * max(1, max|ref|) over the kind's channels; tol 1e-4 (f32), 2e-2 (bf16)
#   mean, running_*             rtol 1e-4, atol 1e-5
#   invstd                      rtol 1e-4, the saved statistics' relative bound.  It holds for bf16 too, whose
#                               per-thread sums are f32 (csrc/bb_nn.hip accumulate): a bf16 square has 16 significant
#                               bits, so a thread's few hundred terms of one magnitude add without rounding in f32's
#                               24, and the sums across threads are fp64
#   dweight, dbias              sums: |err| <= 1e-5 * sum|terms| (tests/test_gpu_linear_tail.py), + 1e-30
#   dpre_bias                   rounding level against dweight: |err| <= 1e-3 * max|dweight| of the tensor
#                               (test_network_fused_conv_bias_batchnorm_matches_torch's form)
NAMES = ("y", "dx", "mean", "invstd", "running_mean", "running_var", "dweight", "dbias", "dpre_bias")


def ratios(got, ref, kinds, bf16):
    """got: dict of fp64 arrays under NAMES (a missing or None entry is skipped) -> {name: {kind: worst ratio}}."""
    tol = 2e-2 if bf16 else 1e-4
    out = {}
    for name in NAMES:
        if got.get(name) is None:
            continue
        a, r = np.asarray(got[name], np.float64), ref[name]
        out[name] = {}
        for kind in sorted(set(kinds.tolist())):
            ch = np.flatnonzero(kinds == kind)
            e, rr = (np.abs(a - r)[:, ch], r[:, ch]) if r.ndim == 4 else (np.abs(a - r)[ch], r[ch])
            if name in ("y", "dx"):
                allowed = tol * max(1.0, float(np.abs(rr).max())) + tol * np.abs(rr)
            elif name == "invstd":
                allowed = 1e-4 * np.abs(rr)
            elif name in ("dweight", "dbias"):
                allowed = 1e-5 * ref["abs_" + name][ch] + 1e-30
            elif name == "dpre_bias":
                allowed = 1e-3 * float(np.abs(ref["dweight"]).max()) + 1e-30
            else:
                allowed = 1e-5 + 1e-4 * np.abs(rr)
            out[name][kind] = float((e / allowed).max())
    return out


def worst(r):
    """{name: (worst ratio, its kind)} of a ``ratios`` result."""
    return {n: max((v, k) for k, v in d.items()) for n, d in r.items()}
