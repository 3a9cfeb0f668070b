"""The bf16 Linear tails of csrc/bb_optim.hip past the workload's shapes: the row counts at which the split
reductions change shape (128 / 129 rows for the bias gradient, 256 / 257 for the weight gradient, 16 / 17 for the
one-output forward), their upper ends (64 chunks that grow past 128 rows above 8,192 rows; 64 splits of 256 at 16,384
rows), column counts that take the non-vector kernel, a misaligned dy, x as a column slice (ldx > K) and
bb_linear_bgrad2 called directly.

The bounds are tests/test_gpu_linear_tail.py's: a sum is within 2^-8 |exact| + 1e-5 sum|terms| of the fp64 sum of the
same bf16 operands (one bf16 rounding of the result plus f32 summation noise); what that module holds bit-exact (g,
dx, repeated calls) is bit-exact here.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16)


def _within(out, exact, absum, what):
    err = (out.double() - exact).abs()
    tol = 2.0 ** -8 * exact.abs() + 1e-5 * absum + 1e-30
    assert out.shape == exact.shape, (what, out.shape, exact.shape)
    assert bool((err <= tol).all()), (what, float((err / tol).max()))


def _bgrad_inputs(cuda, rows, cols, masked, offset=0):
    g0 = torch.Generator(device=cuda).manual_seed(rows * 131 + cols + offset)
    buf = _bf(torch.randn(rows * cols + 8, device=cuda, generator=g0))
    gy = buf[offset:offset + rows * cols].view(rows, cols)
    yd = None
    if masked:
        yd = _bf(torch.randn((rows, cols), device=cuda, generator=g0)).clamp_min(0)
        yd[::7] = 0.0
        yd[:, ::5] = -0.0
    return gy, yd


def _check_bgrad(gy, yd, scale, g, db, what):
    if yd is not None:
        ref = torch.where(yd > 0, _bf(gy.float() * scale), torch.zeros_like(gy))
        assert torch.equal(g, ref), what
    else:
        ref = gy
        assert g.data_ptr() == gy.data_ptr()
    assert db.dtype == torch.bfloat16
    _within(db, ref.double().sum(0), ref.double().abs().sum(0), what)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 8192, 8193, 16384])
def test_linear_bgrad_rows_and_columns(cuda, rows, masked):
    from runtime import kernels as K

    for cols in (8, 64, 72, 100):  # one lane, one full block, a partial second block, the non-vector kernel
        gy, yd = _bgrad_inputs(cuda, rows, cols, masked)
        scale = 1 / 0.9 if masked else 1.0
        g, db = K.linear_bgrad(gy, yd, scale)
        _check_bgrad(gy, yd, scale, g, db, (rows, cols))
        g2, db2 = K.linear_bgrad(gy, yd, scale)
        assert torch.equal(db, db2) and torch.equal(g, g2)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rows", [129, 8193])
def test_linear_bgrad_misaligned_dy_takes_the_scalar_kernel(cuda, rows, masked):
    """dy one bf16 past a 16-byte boundary with 64 columns (cols % 8 == 0, so only the pointer rules out the vector
    kernel): g and db follow the same rules."""
    from runtime import kernels as K

    gy, yd = _bgrad_inputs(cuda, rows, 64, masked, offset=1)
    assert gy.data_ptr() % 16 == 2 and gy.is_contiguous()
    g, db = K.linear_bgrad(gy, yd, 1.25)
    _check_bgrad(gy, yd, 1.25, g, db, (rows, "misaligned"))
    aligned = gy.clone()
    g1, db1 = K.linear_bgrad(aligned, yd, 1.25)  # the vector kernel adds in the same order
    assert torch.equal(db, db1) and torch.equal(g, g1)


def test_linear_bgrad_shapes_in_turn_on_one_stream_leave_the_counters_armed(cuda):
    from runtime import kernels as K

    for rows, cols in ((8193, 64), (37, 24), (2048, 512), (8193, 64)):
        gy, yd = _bgrad_inputs(cuda, rows, cols, True)
        g, db = K.linear_bgrad(gy, yd, 1 / 0.9)
        _check_bgrad(gy, yd, 1 / 0.9, g, db, (rows, cols))
    torch.cuda.synchronize()
    blocks = K.counter_blocks()
    assert blocks and all(int(b.abs().sum()) == 0 for b in blocks)


@pytest.mark.parametrize("rows", [129, 8193])
@pytest.mark.parametrize("cols,split", [(64, 8), (64, 56), (64, 32), (136, 8), (136, 128), (136, 64), (136, 72)])
def test_linear_bgrad2_equals_bgrad_on_the_concatenation(cuda, rows, cols, split):
    """Splits of 8, cols - 8 and about half (at 136 columns cols / 2 = 68 is not a multiple of 8 and is refused below:
    64 and 72 stand either side of it)."""
    from runtime import kernels as K

    g0 = torch.Generator(device=cuda).manual_seed(rows + cols + split)
    gy = _bf(torch.randn((rows, split), device=cuda, generator=g0))
    gy2 = _bf(torch.randn((rows, cols - split), device=cuda, generator=g0))
    yd = _bf(torch.randn((rows, cols), device=cuda, generator=g0)).clamp_min(0)
    yd[::7] = 0.0
    yd[:, ::5] = -0.0
    g, db = K.linear_bgrad2(gy, gy2, yd)
    cat = torch.cat([gy, gy2], 1)
    g1, db1 = K.linear_bgrad(cat, yd, 1.0)
    assert torch.equal(g, g1) and torch.equal(db, db1)
    _check_bgrad(cat, yd, 1.0, g, db, (rows, cols, split))


def test_linear_bgrad2_refuses_odd_and_misaligned_splits(cuda):
    from runtime import kernels as K
    from runtime import lib as L

    rows = 129
    yd = torch.ones((rows, 136), dtype=torch.bfloat16, device=cuda)
    for split in (68, 12, 4, 132):  # split % 8 or (cols - split) % 8
        gy = torch.ones((rows, split), dtype=torch.bfloat16, device=cuda)
        gy2 = torch.ones((rows, 136 - split), dtype=torch.bfloat16, device=cuda)
        with pytest.raises(L.BBNativeError):
            K.linear_bgrad2(gy, gy2, yd)
    buf = torch.ones(rows * 64 + 8, dtype=torch.bfloat16, device=cuda)
    gy = buf[1:1 + rows * 64].view(rows, 64)  # a misaligned first source
    gy2 = torch.ones((rows, 72), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(L.BBNativeError):
        K.linear_bgrad2(gy, gy2, yd)
    with pytest.raises(L.BBNativeError):
        K.linear_bgrad2(gy2, gy, yd[:, :136])  # a misaligned second source
    torch.cuda.synchronize()
    assert all(int(b.abs().sum()) == 0 for b in K.counter_blocks())


def _wgrad_check(dw, g, x, what):
    gd, xd = g.double(), x.double()
    _within(dw, gd.t().mm(xd), gd.abs().t().mm(xd.abs()), what)


@pytest.mark.parametrize("n,k", [(32, 32), (64, 96)])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 16384])
def test_linear_wgrad_rows_and_a_column_slice(cuda, rows, n, k):
    from runtime import kernels as K

    g0 = torch.Generator(device=cuda).manual_seed(rows + n + k)
    g = _bf(torch.randn((rows, n), device=cuda, generator=g0))
    wide = _bf(torch.randn((rows, k + 32), device=cuda, generator=g0))
    x = wide[:, 8:8 + k]
    assert x.stride(0) == k + 32 and K._rows_ok(x)
    dw = K.linear_wgrad(g, x)
    assert dw.shape == (n, k) and dw.dtype == torch.bfloat16
    _wgrad_check(dw, g, x, (rows, n, k))
    assert torch.equal(dw, K.linear_wgrad(g, x))
    assert torch.equal(dw, K.linear_wgrad(g, x.contiguous()))  # ldx changes addresses only


def test_linear_wgrad_past_its_row_limit_falls_back_and_is_still_right(cuda):
    from runtime import kernels as K

    g0 = torch.Generator(device=cuda).manual_seed(5)
    g = _bf(torch.randn((16385, 32), device=cuda, generator=g0))
    x = _bf(torch.randn((16385, 32), device=cuda, generator=g0))
    assert K.L.load().bb_linear_wgrad_workspace_bytes(16385, 32, 32) == -1
    _wgrad_check(K.linear_wgrad(g, x), g, x, "fallback")
    torch.cuda.synchronize()
    assert all(int(b.abs().sum()) == 0 for b in K.counter_blocks())


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 8193])
def test_linear_n1_rows_widths_and_a_column_slice(cuda, rows, bias):
    from runtime import kernels as K

    for k in (8, 128, 136, 256):  # one lane, one pass of 16 lanes, a second pass, two column blocks backward
        g0 = torch.Generator(device=cuda).manual_seed(rows * 7 + k)
        wide = _bf(torch.randn((rows, k + 32), device=cuda, generator=g0))
        x0 = wide[:, 8:8 + k]
        w0 = _bf(torch.randn((1, k), device=cuda, generator=g0) * 0.1)
        b0 = _bf(torch.randn(1, device=cuda, generator=g0)) if bias else None
        gy = _bf(torch.randn((rows, 1), device=cuda, generator=g0))
        x = x0.detach().requires_grad_(True)
        assert x.stride(0) == k + 32 and x.data_ptr() % 16 == 0
        w = w0.clone().requires_grad_(True)
        b = b0.clone().requires_grad_(True) if bias else None
        y = K.LinearN1Function.apply(x, w, b)
        xd, wd = x0.double(), w0.double()
        exact = xd.mm(wd.t()) + (b0.double() if bias else 0.0)
        absum = xd.abs().mm(wd.abs().t()) + (b0.double().abs() if bias else 0.0)
        _within(y, exact, absum, ("y", rows, k))
        y.backward(gy)
        assert torch.equal(x.grad, _bf(gy.float() * w0.float())), ("dx", rows, k)
        _within(w.grad, gy.double().t().mm(xd), gy.double().abs().t().mm(xd.abs()), ("dW", rows, k))
        if bias:
            _within(b.grad, gy.double().sum(0), gy.double().abs().sum(0), ("db", rows, k))
    torch.cuda.synchronize()
    assert all(int(c.abs().sum()) == 0 for c in K.counter_blocks())
