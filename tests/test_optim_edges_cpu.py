"""tests/_optim_ref.py without a GPU: the fp64 Adam restatement is torch's own clip_grad_norm_ + Adam in float64 (so
the GPU tests compare against torch's algorithm, not ours), the catalogue holds every size, alignment variant, state
and gradient kind and stays fair to fp32, bf16_rne is torch's CPU cast bit for bit, dropout_ref draws the right share
and feels every word of seed and offset; and the host-only entry points of libbbvec.so (workspace sizes and counter
counts of csrc/bb_optim.hip) sit at their documented edges.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _optim_ref as R


def test_adam_reference_is_torch_float64():
    rng = np.random.default_rng(3)
    shapes = [(7,), (3, 5), (40,)]
    p0 = [rng.standard_normal(s) for s in shapes]
    params = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p0]
    opt = torch.optim.Adam(params, lr=R.LR, betas=(R.BETA1, R.BETA2), eps=R.EPS)
    p, m, v = p0, [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    steps = [0.0] * len(shapes)
    for k, max_norm in enumerate((0.5, 1e9, 0.5)):  # clipped, not clipped, clipped
        g = [rng.standard_normal(s) * (1.0, 1.0, 0.01)[k] for s in shapes]
        for q, x in zip(params, g):
            q.grad = torch.from_numpy(x.copy())
        tn = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        r = R.adam_clip_ref(p, g, m, v, steps, R.LR, R.BETA1, R.BETA2, R.EPS, max_norm)
        assert (r["coef"] < 1.0) == (k == 0)  # the small gradients of step 2 stay under max_norm
        np.testing.assert_allclose(r["norm64"], float(tn), rtol=1e-12)
        for i, q in enumerate(params):
            st = opt.state[q]
            np.testing.assert_allclose(r["g"][i], q.grad.numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(r["m"][i], st["exp_avg"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(r["v"][i], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(r["p"][i], q.detach().numpy(), rtol=1e-12, atol=0)
            # (p ~ 1: the difference cancels)
            np.testing.assert_allclose(r["upd64"][i], p[i] - r["p"][i], rtol=0, atol=1e-15)
            assert r["step"][i] == float(st["step"]) == k + 1
        p, m, v, steps = r["p"], r["m"], r["v"], r["step"]


def test_adam_replay_rounds_where_the_kernel_does():
    """With norm32 the restatement's g', m', v' are fp32 values, within fp32 rounding of the exact ones."""
    rng = np.random.default_rng(4)
    p, g, m, v = (rng.standard_normal(100).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    ex = R.adam_clip_ref([p], [g], [m], [v], [9.0], R.LR, R.BETA1, R.BETA2, R.EPS, 0.5)
    rp = R.adam_clip_ref([p], [g], [m], [v], [9.0], R.LR, R.BETA1, R.BETA2, R.EPS, 0.5, np.float32(ex["norm64"]))
    assert type(rp["coef"]) is np.float32 and rp["coef"] < 1
    for k in ("g", "m", "v"):
        assert np.array_equal(rp[k][0], rp[k][0].astype(np.float32).astype(np.float64))
        np.testing.assert_allclose(rp[k][0], ex[k][0], rtol=4 * 2.0 ** -24, atol=1e-9)
    np.testing.assert_allclose(rp["p"][0], ex["p"][0], rtol=0, atol=1e-9)


def test_catalogue_holds_every_size_alignment_state_and_gradient():
    cases = R.adam_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in cases}
    assert sorted(names) == sorted(
        [f"sizes-{a}" for a in R.ALIGNS] + ["table48", "mixed-align"] + [f"chunks{k}" for k in R.CHUNK_TOTALS]
        + [f"state-{s}" for s in R.STATES[1:]]
        + ["grad-zero", "grad-mixed", "grad-single0.25", "grad-single0.5", "max-norm-1e9"])
    assert sorted(R.ALIGNS) == ["aligned", "all1", "g1", "g2", "g3", "m1"]
    for a, offs in R.ALIGNS.items():
        c = by[f"sizes-{a}"]
        assert c.sizes == (1, 3, 4, 5, 2047, 2048, 2049, 4096, 4097, 6143) and set(c.aligns) == {a}
        starts, totals = R.layout(c)
        for b in range(4):
            assert [s % 4 for s in starts[b]] == [offs[b]] * len(c.sizes)
    assert R.ALIGNS["all1"] == (1, 1, 1, 1) and R.ALIGNS["m1"] == (0, 0, 1, 0)
    assert [R.ALIGNS[f"g{i}"] for i in (1, 2, 3)] == [(0, i, 0, 0) for i in (1, 2, 3)]
    assert {c.state for c in cases} == set(R.STATES) and {c.grad for c in cases} == set(R.GRADS)
    assert {c.max_norm for c in cases} == {0.5, 1e9}
    # the table limit, with a partial last chunk and every alignment variant inside one launch
    t = by["table48"]
    assert len(t.sizes) == R.MAX_TENSORS == 48 and t.sizes[-1] % R.CHUNK and t.sizes[-1] > R.CHUNK
    assert set(t.aligns) == set(R.ALIGNS) and len(set(t.sizes)) >= 8
    assert set(by["mixed-align"].aligns) == set(R.ALIGNS)
    # the finaliser's 8-wide loop edge (i + 7 * 256 < nchunks) and one pass of every loop
    for k in (2047, 2048, 2049):
        assert by[f"chunks{k}"].sizes == (2048 * k - 5,) and R.chunk_total(by[f"chunks{k}"]) == k
    assert R.chunk_total(by["chunks2305"]) == 2048 + 256 + 1 and len(by["chunks2305"].sizes) == 2
    # guards: at least 4 sentinel floats between neighbours and at both ends of all four buffers
    for c in cases:
        starts, totals = R.layout(c)
        for b in range(4):
            end = 0
            for s, n in zip(starts[b], c.sizes):
                assert s - end >= R.GUARD
                end = s + n
            assert totals[b] - end >= R.GUARD and totals[b] % 4 == 0


@pytest.mark.parametrize("case", [c for c in R.adam_cases()], ids=lambda c: c.name)
def test_catalogue_case_is_what_it_is_named_for_and_fair_to_fp32(case):
    R.check_fair(case)
    b = R.build(case)
    st, sz = b["starts"], case.sizes
    for k in "pmv":
        assert not R.guards_intact(b["flat"][k], [s + 1 for s in st["pgmv".index(k)]], sz)  # the check can fail
        assert R.guards_intact(b["flat"][k], st["pgmv".index(k)], sz)
    g = R.gradients(case, 0)
    m = R.views(b["flat"]["m"], st[2], sz)
    v = R.views(b["flat"]["v"], st[3], sz)
    assert b["steps"] == [float(case.state.split("@")[1])] * len(sz)
    if case.state == "zero@0":
        assert not any(x.any() for x in m) and not any(x.any() for x in v)
    else:
        gm = np.concatenate(g) * np.concatenate(m)
        if case.grad != "zero":
            assert 0.3 < float((gm < 0).mean()) < 0.7 or gm.size < 8  # opposite in sign on half
        ratio = np.concatenate(v).astype(np.float64) / np.maximum(np.concatenate(g).astype(np.float64) ** 2, 1e-300)
        if case.grad == "normal" and case.max_norm == 0.5:  # against the clipped size (about 1e-2 of g)
            assert (ratio > 1e2).any() and (ratio < 1e-10).any()
        assert all((x > 0).all() for x in v) and all(x.all() for x in m)
    if case.grad == "zero":
        assert not any(x.any() for x in g) and all(x.all() for x in m)
    if case.grad == "mixed":
        mags = sorted(float(np.abs(x).max()) for x in g)
        assert mags[0] < 1.1e-12 and 0.5 < mags[1] <= 1.0 and mags[2] > 5e5
    if case.grad.startswith("single"):
        r = R.adam_clip_ref(R.views(b["flat"]["p"], st[0], sz), g, m, v, b["steps"], R.LR, R.BETA1, R.BETA2, R.EPS,
                            case.max_norm, np.float32(g[0][0]))
        assert (r["coef"] == 1.0) == (case.grad == "single0.25")
        assert 1.0 - 1e-5 < r["coef"] <= 1.0


def test_bf16_rne_is_torch_cpu_cast():
    bits = R.cast_patterns()
    assert bits.size == 4 * 65536 + 28 and bits.dtype == np.uint32
    x = torch.from_numpy(bits.view(np.float32).copy())
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_rne(bits.view(np.float32))
    nan = np.isnan(bits.view(np.float32))
    assert np.array_equal(R.is_nan_bf16(got), nan) and np.array_equal(R.is_nan_bf16(want), nan)
    assert np.array_equal(got[~nan], want[~nan])
    # the set holds what it is for: ties on even and odd mantissas, subnormals, the overflow to infinity
    f = lambda b: R.bf16_rne(np.array([b], np.uint32).view(np.float32))[0]  # noqa: E731
    assert f(0x3F808000) == 0x3F80 and f(0x3F818000) == 0x3F82 and f(0x3F808001) == 0x3F81
    assert f(0x7F7FFFFF) == 0x7F80 and f(0x00008000) == 0x0000 and f(0x00018000) == 0x0002
    assert R.is_nan_bf16(f(0x7F800001)) and R.is_nan_bf16(f(0x7FFFFFFF))
    for b in (0x3F808000, 0x3F818000, 0x00000001, 0x7F7FFFFF, 0x7F800001, 0x80000000):
        assert b in bits


def test_dropout_reference_share_and_high_words():
    n = 1 << 20
    HI = 1 << 32
    for p in (0.1, 0.5):
        keep, scale = R.dropout_ref(n, p, 12345, 0)
        assert abs((1.0 - keep.mean()) - p) < 5 * (p * (1 - p) / n) ** 0.5
        assert scale == np.float32(1.0 / float(np.float32(1.0 - float(np.float32(p)))))
    base, _ = R.dropout_ref(4096, 0.5, 12345, 0)
    for seed, off in ((3 * HI + 12345, 0), (12345, 9 * HI + 7), (12345, 7), (HI - 1, HI - 1), (12345, HI)):
        other, _ = R.dropout_ref(4096, 0.5, seed, off)
        assert 0.3 < float((other != base).mean()) < 0.7, (seed, off)
    assert R.dropout_ref(64, 1e-10, 1, 0)[0].all()  # threshold 0
    assert R.dropout_ref(64, 1e-10, 1, 0)[1] == np.float32(1.0)
    # the four words of one counter go to four neighbouring elements
    from oracle.philox import philox4x32_10

    w = philox4x32_10(np.array([5], np.uint64), 7, 12345)
    keep, _ = R.dropout_ref(24, 0.5, 12345, 7)
    assert keep[20:24].tolist() == [bool(x[0] >= 0x80000000) for x in w]


# ---------------------------------------------------------------------------------------------------------------
# Host-only entry points of libbbvec.so against the constants of csrc/bb_optim.hip
# ---------------------------------------------------------------------------------------------------------------
def _numel(ns):
    return (C.c_int64 * len(ns))(*ns)


def test_adam_workspace_bytes(lib):
    for ns in ([1], [2048], [2049], [5, 2048, 4097], [1] * 48, [2048 * 2049 - 5]):
        chunks = sum(-(-n // 2048) for n in ns)
        assert lib.bb_adam_clip_workspace_bytes(len(ns), _numel(ns)) == (8 + 48 + chunks) * 8
    assert lib.bb_adam_clip_workspace_bytes(0, None) == -1
    assert lib.bb_adam_clip_workspace_bytes(49, _numel([4] * 49)) == -1
    assert lib.bb_adam_clip_workspace_bytes(2, _numel([4, 0])) == -1
    assert lib.bb_adam_clip_workspace_bytes(1, _numel([-3])) == -1


@pytest.mark.parametrize("rows,split", [(1, 1), (128, 1), (129, 2), (8192, 64), (8193, 64), (16384, 64)])
def test_linear_bgrad_workspace_bytes(lib, rows, split):
    for cols, blocks in ((1, 1), (64, 1), (65, 2), (100, 2), (512, 8)):
        assert lib.bb_linear_bgrad_workspace_bytes(rows, cols) == blocks * split * 64 * 4
        assert lib.bb_linear_bgrad_counters(cols) == blocks
    assert lib.bb_linear_bgrad_workspace_bytes(0, 64) == -1 and lib.bb_linear_bgrad_workspace_bytes(rows, 0) == -1
    assert lib.bb_linear_bgrad_counters(0) == -1


@pytest.mark.parametrize("rows,split", [(1, 1), (256, 1), (257, 2), (16384, 64)])
def test_linear_wgrad_workspace_bytes(lib, rows, split):
    for n, k in ((32, 32), (64, 96), (512, 512)):
        tiles = (n // 32) * (k // 32)
        assert lib.bb_linear_wgrad_workspace_bytes(rows, n, k) == tiles * split * 32 * 32 * 4
        assert lib.bb_linear_wgrad_counters(n, k) == tiles
    assert lib.bb_linear_wgrad_workspace_bytes(16385, 32, 32) == -1
    assert lib.bb_linear_wgrad_workspace_bytes(0, 32, 32) == -1
    for n, k in ((33, 32), (32, 48), (16, 32), (32, 8)):
        assert lib.bb_linear_wgrad_workspace_bytes(rows, n, k) == -1
        assert lib.bb_linear_wgrad_counters(n, k) == -1


@pytest.mark.parametrize("rows,split", [(1, 1), (128, 1), (129, 2), (8192, 64), (8193, 64)])
def test_linear_n1_workspace_bytes(lib, rows, split):
    for k, blocks in ((8, 1), (64, 1), (72, 2), (128, 2), (136, 3), (256, 4)):
        assert lib.bb_linear_n1_workspace_bytes(rows, k) == blocks * split * 65 * 4
        assert lib.bb_linear_n1_counters(k) == blocks
    for k in (0, 4, 12, 129):
        assert lib.bb_linear_n1_workspace_bytes(rows, k) == -1
        assert lib.bb_linear_n1_counters(k) == -1
    assert lib.bb_linear_n1_workspace_bytes(0, 8) == -1
