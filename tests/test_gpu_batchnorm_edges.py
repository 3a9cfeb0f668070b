"""bb_bn_forward / bb_bn_backward (runtime.kernels.BatchNormReLUFunction) on the MI355X against the fp64 restatement of
tests/_bn_ref.py, with the channel kinds mixed inside one tensor: unit N(0, 1); offset (mean 8, std 0.25: the mean is
32 standard deviations out); const (every element 0.5: var = 0, everything scaled by 1/sqrt(eps) = 316); tiny (std 1e-3:
the variance is far below eps); big (std 1e3); dead (weight 0.01, bias -5 under the ReLU: every output and gradient 0).

Shapes (_bn_ref.cases): N in {1, 3, 33, 257} at 8x8, NCHW and channels_last, f32 and bf16, the ReLU on and off, C in
{4, 8, 64, 128} as the layout and dtype allow, pre_bias absent and around 100 (the statistics are bias-free, the running
mean is not), momentum 0.1 and 0.25; NCHW rows of 2x2, 4x4, 6x6, 16x16 and 32x32 (the largest legal row), NHWC at 6x6 and
2x2.  Every bound (_bn_ref.ratios) is asserted per channel kind; every case prints the kernel's worst ratio to its bound
beside that of torch's own fp32 nn.BatchNorm2d on the same device and values.

A (2, 8, 64, 64) f32 input is beyond the NCHW row limit of include/bbvec.h: models.network.BatchNorm2d hands it to
torch, where bb_bn_workspace_bytes once divided by zero.
"""
import numpy as np
import pytest
import torch

import _bn_ref as B

pytestmark = pytest.mark.gpu

EPS = 1e-5
CASES = B.cases()


def _dev(a, case, dev, act=False):
    """A fp64 array on the device: activations in the case's dtype and layout, parameters f32."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if not act:
        return t.float()
    t = t.to(torch.bfloat16 if case.bf16 else torch.float32)
    return t.contiguous(memory_format=torch.channels_last) if case.nhwc else t.contiguous()


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _fused(case, inp, dev):
    from runtime import kernels as K

    x = _dev(inp["x"], case, dev, act=True).requires_grad_(True)
    dy = _dev(inp["dy"], case, dev, act=True)
    w, b = _dev(inp["weight"], case, dev).requires_grad_(True), _dev(inp["bias"], case, dev).requires_grad_(True)
    pb = _dev(inp["pre_bias"], case, dev).requires_grad_(True) if case.pre_bias else None
    rm, rv = _dev(inp["running_mean"], case, dev), _dev(inp["running_var"], case, dev)
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    assert K.bn_fusable(x)
    y = K.BatchNormReLUFunction.apply(x, pb, w, b, rm, rv, case.momentum, EPS, case.relu, nbt)
    assert y.dtype == x.dtype and y.shape == x.shape
    assert y.is_contiguous(memory_format=torch.channels_last if case.nhwc else torch.contiguous_format)
    saved = y.grad_fn.saved_tensors
    y.backward(dy)
    torch.cuda.synchronize(dev)
    assert int(nbt) == 6
    assert x.grad.dtype == x.dtype and w.grad.dtype == torch.float32
    got = {"y": y, "mean": saved[4], "invstd": saved[5], "running_mean": rm, "running_var": rv, "dx": x.grad,
           "dweight": w.grad, "dbias": b.grad, "dpre_bias": pb.grad if pb is not None else None}
    return {k: _np(v) for k, v in got.items()}, x.detach(), dy, (w.detach(), b.detach())


def _torch_fp32(case, inp, x, dy, wb, mask, dev):
    """nn.BatchNorm2d in fp32 on the stored values (bias-free, as the kernel's statistics; the bias goes into the
    running mean afterwards in fp64), its backward under the same mask."""
    m = torch.nn.BatchNorm2d(case.c, eps=EPS, momentum=case.momentum).to(dev).train()
    with torch.no_grad():
        m.weight.copy_(wb[0])
        m.bias.copy_(wb[1])
        m.running_mean.copy_(_dev(inp["running_mean"], case, dev))
        m.running_var.copy_(_dev(inp["running_var"], case, dev))
    xr = x.float().contiguous().requires_grad_(True)
    yr = m(xr)
    g = dy.float().contiguous()
    yr.backward(g * mask if case.relu else g)
    rmean = _np(m.running_mean) + (case.momentum * inp["pre_bias"] if case.pre_bias else 0.0)
    return {"y": _np(torch.relu(yr) if case.relu else yr), "running_mean": rmean,
            "running_var": _np(m.running_var), "dx": _np(xr.grad), "dweight": _np(m.weight.grad),
            "dbias": _np(m.bias.grad)}


@pytest.mark.parametrize("case", CASES, ids=[B.case_id(k) for k in CASES])
def test_batchnorm_matches_fp64_per_channel_kind(cuda, case):
    inp = B.inputs(case)
    kinds = inp["kinds"]
    got, x, dy, wb = _fused(case, inp, cuda)
    mask = torch.from_numpy(got["y"] > 0).to(cuda) if case.relu else None
    ref = B.reference(_np(x), _np(dy), _np(wb[0]), _np(wb[1]),
                      _np(_dev(inp["pre_bias"], case, cuda)) if case.pre_bias else None,
                      _np(_dev(inp["running_mean"], case, cuda)), _np(_dev(inp["running_var"], case, cuda)),
                      case.momentum, EPS, case.relu, mask=(got["y"] > 0) if case.relu else None)
    rk = B.ratios(got, ref, kinds, case.bf16)
    rt = B.ratios(_torch_fp32(case, inp, x, dy, wb, mask, cuda), ref, kinds, case.bf16)
    wk, wt = B.worst(rk), B.worst(rt)
    print(f"\n{B.case_id(case)}: worst |err| / bound, kernel (torch fp32) -- "
          + " ".join(f"{n} {wk[n][0]:.3g}@{wk[n][1]}" + (f" ({wt[n][0]:.3g}@{wt[n][1]})" if n in wt else "")
                     for n in B.NAMES if n in wk))
    if case.relu and "dead" in kinds:
        d = kinds == "dead"
        assert not got["y"][:, d].any() and not got["dx"][:, d].any()
        assert not got["dweight"][d].any() and not got["dbias"][d].any()
    if "const" in kinds:
        c = kinds == "const"
        assert (got["mean"][c] == 0.5).all()  # the sums of 0.5 and 0.25 are exact at these sizes: var = 0
        assert np.allclose(got["invstd"][c], 1.0 / np.sqrt(EPS), rtol=1e-6, atol=0)
    bad = [(n, k, v) for n, d in rk.items() for k, v in d.items() if not v <= 1.0]
    assert not bad, bad


def test_rows_beyond_the_nchw_limit_go_through_torch(cuda):
    from models.network import BatchNorm2d
    from runtime.kernels import bn_fusable

    torch.manual_seed(64)
    x0 = torch.randn(2, 8, 64, 64, device=cuda) * 1.7 + 0.3
    assert not bn_fusable(x0) and not bn_fusable(x0[:, :, :, :40].bfloat16().contiguous())  # 4 x 4096, 2 x 2560 bytes
    assert bn_fusable(x0[:, :, :32, :32].contiguous()) and bn_fusable(x0[:, :, :, :32].bfloat16().contiguous())
    ref = torch.nn.BatchNorm2d(8).to(cuda).train()
    fus = BatchNorm2d(8, relu=True).to(cuda).train()
    with torch.no_grad():
        for m in (ref, fus):
            m.weight.copy_(torch.linspace(0.5, 1.5, 8))
            m.bias.copy_(torch.linspace(-0.2, 0.2, 8))
    g = torch.randn_like(x0)
    xf, xr = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    yf, yr = fus(xf), torch.relu(ref(xr))
    yf.backward(g)
    yr.backward(g)
    for a, b in ((yf, yr), (xf.grad, xr.grad), (fus.weight.grad, ref.weight.grad), (fus.bias.grad, ref.bias.grad),
                 (fus.running_mean, ref.running_mean), (fus.running_var, ref.running_var)):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)  # torch's own kernels on both sides
    assert int(fus.num_batches_tracked) == 1
