"""The bf16 3x3 forward kernel (csrc/bb_conv.hip, conv_fwd_kernel) and its fused variants on integer data, bit for bit.

Activations, gradients and weights are small integers (tests/_conv_ref.py, the *small* and *wide* families), so every
product and every partial sum is exact in fp32 whatever the order and the MFMA shape (tests/test_conv_edges_cpu.py
shows the bounds).  The forward and the data gradient (the same kernel over dy with the wd image) must then equal the
float64 restatement rounded once to bf16, nearest even, in every element; bb_conv3x3_forward_add must equal
bf16(bf16(conv) + add); the statistics partials of bb_conv3x3_forward_stats / _bstats must equal the exact sums per
workgroup (2 boards), which for an odd batch pins that the last workgroup's phantom board counts nothing.  Every
output is a view into a larger sentinel-filled buffer, at least one board on each side: a store for the phantom board
would land in the guard.

The reference of a (pair, family) is computed once at the largest batch; the smaller batches are its first boards
(the inputs of board b do not depend on the batch size, and boards do not interact).
"""
import numpy as np
import pytest
import torch

import _conv_ref as CR

pytestmark = pytest.mark.gpu

NBS = CR.FWD_NB
NBMAX = max(NBS)
_cache = {}


def _ref(cuda, cin, cout, fam):
    """x, w, g (CPU; x and g kept as int8, their values are that small) and the bf16 bit patterns of y = conv(x, w)
    and dx = dgrad(g, w) at NBMAX boards."""
    key = (cin, cout, fam)
    if key not in _cache:
        x, w, g = CR.int_x(fam, NBMAX, cin), CR.int_w(fam, cin, cout), CR.int_g(fam, NBMAX, cout)
        y = CR.conv_forward(x.to(cuda), w.to(cuda))
        dx = CR.conv_dgrad(g.to(cuda), w.to(cuda))
        _cache[key] = (x.to(torch.int8), w, g.to(torch.int8), CR.bf16_bits(y), CR.bf16_bits(dx),
                       int(CR.is_tie(y).sum()) + int(CR.is_tie(dx).sum()))
    return _cache[key]


def _images(lib, cuda, w, wl):
    """bb_conv3x3_prep's (wf, wd) of the float64 weight [cout, cin, 3, 3], handed over in layout wl."""
    from runtime import kernels as K

    cout, cin = w.shape[:2]
    wdev = (w.permute(0, 2, 3, 1) if wl else w).contiguous().to(cuda).float().view(-1)
    wf = torch.empty(9 * cin * cout, dtype=torch.bfloat16, device=cuda)
    wd = torch.empty_like(wf)
    K.L.check(lib.bb_conv3x3_prep(K._p(wdev), cin, cout, wl, K._p(wf), K._p(wd), K._s(cuda)), "prep")
    return wf, wd


def _out(cuda, nb, c):
    pad = 2 * 64 * c  # two boards of the output's rows on each side
    flat, view = CR.guarded(cuda, torch.bfloat16, nb * 64 * c, pad)
    return flat, view, pad


def _check_out(flat, view, pad, want_bits, what):
    got = CR.bits16(view)
    want = np.asarray(want_bits).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[:5]}"
    assert CR.guards_ok(flat, view.numel(), pad), f"{what}: a store outside the output"


def _forward(lib, cuda, x, w_img, nb, cin, cout, view):
    from runtime import kernels as K

    K.L.check(lib.bb_conv3x3_forward(K._p(x), K._p(w_img), nb, cin, cout, K._p(view), K._s(cuda)), "forward")


@pytest.mark.parametrize("fam", CR.FAMILIES)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_forward_and_data_gradient_bit_exact(cuda, lib, cin, cout, nb, fam):
    x, w, g, ybits, dxbits, ties = _ref(cuda, cin, cout, fam)
    if fam == "wide":
        assert ties >= 1000  # the rounding is exercised on exact ties
    wf, wd = _images(lib, cuda, w, nb % 2)
    flat, view, pad = _out(cuda, nb, cout)
    _forward(lib, cuda, CR.nhwc_bf16(x[:nb], cuda), wf, nb, cin, cout, view)
    _check_out(flat, view, pad, ybits[:nb], "forward")
    flat, view, pad = _out(cuda, nb, cin)
    _forward(lib, cuda, CR.nhwc_bf16(g[:nb], cuda), wd, nb, cout, cin, view)
    _check_out(flat, view, pad, dxbits[:nb], "data gradient")


@pytest.mark.parametrize("nb", [3, 66])
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_one_hot_taps_forward_and_data_gradient(cuda, lib, cin, cout, nb):
    """Integer one-hot weights on every tap (output channel co reads tap co % 9 of one input channel): each output is
    one input value times 1 + tap, so a reversed tap order, a transposed image or a wrong zero row moves values."""
    w = CR.one_hot_w(cin, cout)
    x = CR.int_x("small", nb, cin) * (1 + torch.arange(64).reshape(1, 8, 8, 1) % 7)  # the pixel shows in the value
    g = CR.int_g("small", nb, cout) * (1 + torch.arange(64).reshape(1, 8, 8, 1) % 5)
    wf, wd = _images(lib, cuda, w, 1 - nb % 2)
    y = CR.conv_forward(x.to(cuda), w.to(cuda))
    dx = CR.conv_dgrad(g.to(cuda), w.to(cuda))
    assert int((y != 0).sum()) > y.numel() // 4 and int((dx != 0).sum()) > dx.numel() // 40
    flat, view, pad = _out(cuda, nb, cout)
    _forward(lib, cuda, CR.nhwc_bf16(x, cuda), wf, nb, cin, cout, view)
    _check_out(flat, view, pad, CR.bf16_bits(y), "one-hot forward")
    flat, view, pad = _out(cuda, nb, cin)
    _forward(lib, cuda, CR.nhwc_bf16(g, cuda), wd, nb, cout, cin, view)
    _check_out(flat, view, pad, CR.bf16_bits(dx), "one-hot data gradient")


@pytest.mark.parametrize("fam", CR.FAMILIES)
@pytest.mark.parametrize("nb", [2, 5])
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_forward_add_rounds_twice(cuda, lib, cin, cout, nb, fam):
    """bb_conv3x3_forward_add == bf16(bf16(conv) + add); an eighth of the addends is +-256 or 384, which puts the
    second rounding on a tie wherever the rounded convolution is an odd integer of the right sign."""
    from runtime import kernels as K

    x, w, _, ybits, _, _ = _ref(cuda, cin, cout, fam)
    gen = torch.Generator().manual_seed(77 + nb + cin)
    add = torch.randint(-2, 3, (nb, 8, 8, cout), generator=gen).double()
    big = torch.tensor([256.0, -256.0, 384.0])[torch.randint(0, 3, add.shape, generator=gen)]
    add = torch.where(torch.randint(0, 8, add.shape, generator=gen) == 0, big, add)
    first = CR.from_bits16(ybits[:nb]).reshape(add.shape)
    total = first + add  # exact in fp32: both are integers below 2^12
    ties = int(CR.is_tie(total).sum())
    assert ties >= 50, ties
    wf, _ = _images(lib, cuda, w, 0)
    flat, view, pad = _out(cuda, nb, cout)
    xd, addd = CR.nhwc_bf16(x[:nb], cuda), CR.nhwc_bf16(add, cuda)
    K.L.check(lib.bb_conv3x3_forward_add(K._p(xd), K._p(wf), nb, cin, cout, K._p(addd), K._p(view), K._s(cuda)),
              "forward_add")
    _check_out(flat, view, pad, CR.bf16_bits(total), "forward_add")


def _partials(cuda, nblk, c):
    pad = 2 * 3 * c  # two workgroups' rows on each side
    flat, view = CR.guarded(cuda, torch.float64, nblk * c * 3, pad)
    return flat, view, pad


def _check_partials(flat, view, pad, nblk, c, want, what):
    assert CR.guards_ok(flat, view.numel(), pad), f"{what}: a partial outside the {nblk} workgroups' rows"
    part = view.view(nblk, c, 3)
    for m, ref in enumerate(want):
        bad = part[:, :, m] != ref  # a sentinel left in place is a NaN: unequal
        assert not bool(bad.any()), (f"{what}: sum {m} differs in {int(bad.sum())} (workgroup, channel) pairs, first "
                                     f"{bad.nonzero()[:4].tolist()}; the last workgroup differs: {bool(bad[-1].any())}")


@pytest.mark.parametrize("fam", CR.FAMILIES)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_forward_stats_exact_per_workgroup(cuda, lib, cin, cout, nb, fam):
    from runtime import kernels as K

    x, w, _, ybits, _, _ = _ref(cuda, cin, cout, fam)
    wf, _ = _images(lib, cuda, w, 0)
    xd = CR.nhwc_bf16(x[:nb], cuda)
    plain = torch.empty(nb * 64 * cout, dtype=torch.bfloat16, device=cuda)
    _forward(lib, cuda, xd, wf, nb, cin, cout, plain)
    nblk = lib.bb_conv3x3_stats_blocks(nb, cout)
    assert nblk == CR.stats_blocks(nb)
    flat, view, pad = _out(cuda, nb, cout)
    pflat, part, ppad = _partials(cuda, nblk, cout)
    K.L.check(lib.bb_conv3x3_forward_stats(K._p(xd), K._p(wf), nb, cin, cout, K._p(view), K._p(part), K._s(cuda)),
              "forward_stats")
    _check_out(flat, view, pad, CR.bits16(plain), "forward_stats y against the plain call")
    _check_out(flat, view, pad, ybits[:nb], "forward_stats y")
    r = CR.from_bits16(ybits[:nb], cuda).reshape(nb, 8, 8, cout)  # the stored values
    want = (CR.per_block(r), CR.per_block(r * r), torch.zeros((nblk, cout), dtype=torch.float64, device=cuda))
    _check_partials(pflat, part, ppad, nblk, cout, want, "forward_stats")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_forward_bstats_exact_per_workgroup(cuda, lib, cin, cout, nb, relu):
    """The data gradient of a cin -> cout layer with the BatchNorm-backward sums of the layer before it (cin
    channels), dyadic BatchNorm operands: {sum g, sum g xhat, sum xhat} exact per workgroup, ReLU arguments of
    exactly 0 counted as off."""
    from runtime import kernels as K

    fam = CR.FAMILIES[(NBS.index(nb) + relu) % 2]
    _, w, g, _, dxbits, _ = _ref(cuda, cin, cout, fam)
    _, wd = _images(lib, cuda, w, 1)
    gd = CR.nhwc_bf16(g[:nb], cuda)
    bn = CR.int_bn(NBMAX, cin)
    bn = bn._replace(bx=bn.bx[:nb])
    bx = CR.nhwc_bf16(bn.bx, cuda)
    mean, invstd, bw, bb = (v.to(cuda).float().contiguous() for v in (bn.mean, bn.invstd, bn.weight, bn.bias))
    plain = torch.empty(nb * 64 * cin, dtype=torch.bfloat16, device=cuda)
    _forward(lib, cuda, gd, wd, nb, cout, cin, plain)
    nblk = lib.bb_conv3x3_stats_blocks(nb, cin)
    flat, view, pad = _out(cuda, nb, cin)
    pflat, part, ppad = _partials(cuda, nblk, cin)
    K.L.check(lib.bb_conv3x3_forward_bstats(K._p(gd), K._p(wd), nb, cout, cin, K._p(view), K._p(bx), K._p(mean),
                                            K._p(invstd), K._p(bw), K._p(bb), relu, K._p(part), K._s(cuda)), "bstats")
    _check_out(flat, view, pad, CR.bits16(plain), "forward_bstats dx against the plain call")
    _check_out(flat, view, pad, dxbits[:nb], "forward_bstats dx")
    r = CR.from_bits16(dxbits[:nb], cuda).reshape(nb, 8, 8, cin)
    t0, t1, t2, arg = CR.bn_backward_terms(r, bn, relu)
    assert int((arg == 0).sum()) > 0
    _check_partials(pflat, part, ppad, nblk, cin, (CR.per_block(t0), CR.per_block(t1), CR.per_block(t2)), "bstats")
