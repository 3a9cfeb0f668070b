"""The bf16 convolutions of csrc/bb_conv.hip restated in torch float64, their launch geometry restated in Python,
integer inputs for which fp32 accumulation is exact, guarded device buffers, and the catalogue of cases the
convolution edge tests run.  It calls none of the code under test and needs no GPU of its own: every function takes
the device from its arguments.

Layout: activations are [nb, 8, 8, C] (NHWC, the kernels' memory order), weights [cout, cin, 3, 3] (nn.Conv2d).

conv_forward / conv_dgrad / conv_wgrad   the 3x3 / pad-1 convolution as nine shifted slices and matmuls (no conv2d)
bf16_bits                                exact fp32 values -> bf16 bit patterns, _optim_ref.bf16_rne (nearest even)
wgrad_geometry ...                       wgrad_chunks / wgrad_bpc / wgrad_used and the input layer's grids
family                                   the *small* and *wide* integer inputs
prep_images_ref                          bb_conv3x3_prep's two images from a weight's bit patterns
guarded / guards_ok                      an output as a view into a sentinel-filled buffer
"""
from collections import namedtuple

import numpy as np
import torch

import _optim_ref as R

PAIRS = ((64, 64), (64, 128), (128, 64), (128, 128))
TAPS = tuple((t // 3 - 1, t % 3 - 1) for t in range(9))  # d_t = (dy, dx) of tap t
F32_EXACT = float(2 ** 24)  # integers below it are exact in fp32, and so is every sum of integers that stays below


# ---------------------------------------------------------------------------------------------------------------
# The convolution in float64
# ---------------------------------------------------------------------------------------------------------------
def shift(a, dy, dx):
    """a [nb, 8, 8, C] -> s[b, r, c] = a[b, r + dy, c + dx], zero where that leaves the board."""
    out = torch.zeros_like(a)
    r0, r1 = max(0, -dy), 8 - max(0, dy)
    c0, c1 = max(0, -dx), 8 - max(0, dx)
    out[:, r0:r1, c0:c1] = a[:, r0 + dy:r1 + dy, c0 + dx:c1 + dx]
    return out


def _f64(a):
    return a.to(torch.float64)


def conv_forward(x, w):
    """y[b, p, co] = sum_{t, ci} x[b, p + d_t, ci] w[co, ci, t]; x [nb, 8, 8, cin], w [cout, cin, 3, 3] -> float64."""
    x, w = _f64(x), _f64(w)
    y = torch.zeros(x.shape[:3] + (w.shape[0],), dtype=torch.float64, device=x.device)
    for t, (dy, dx) in enumerate(TAPS):
        y += torch.matmul(shift(x, dy, dx), w[:, :, t // 3, t % 3].t())
    return y


def conv_dgrad(g, w):
    """dx[b, q, ci] = sum_{t, co} g[b, q - d_t, co] w[co, ci, t]; g [nb, 8, 8, cout] -> [nb, 8, 8, cin] float64."""
    g, w = _f64(g), _f64(w)
    dx_ = torch.zeros(g.shape[:3] + (w.shape[1],), dtype=torch.float64, device=g.device)
    for t, (dy, dx) in enumerate(TAPS):
        dx_ += torch.matmul(shift(g, -dy, -dx), w[:, :, t // 3, t % 3])
    return dx_


def conv_wgrad(x, g, absolute=False):
    """dw[co, ci, t] = sum_{b, p} g[b, p, co] x[b, p + d_t, ci] -> [cout, cin, 3, 3] float64; ``absolute``: the sum
    of the terms' magnitudes instead (what an error bound scales with)."""
    x, g = _f64(x), _f64(g)
    if absolute:
        x, g = x.abs(), g.abs()
    cin, cout = x.shape[3], g.shape[3]
    dw = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, device=x.device)
    gt = g.reshape(-1, cout).t()
    for t, (dy, dx) in enumerate(TAPS):
        dw[:, :, t // 3, t % 3] = torch.matmul(gt, shift(x, dy, dx).reshape(-1, cin))
    return dw


def bf16_bits(a):
    """A tensor of values exact in fp32 -> numpy uint16 bf16 patterns, rounded to nearest even (R.bf16_rne)."""
    f = a.to(torch.float32)
    assert bool((f.to(torch.float64) == _f64(a)).all()), "reference values must be exact in fp32"
    return R.bf16_rne(f.cpu().numpy())


def from_bits16(h, device="cpu"):
    """numpy uint16 bf16 patterns -> the values, float64."""
    f = (np.asarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return torch.from_numpy(f.astype(np.float64)).to(device)


def bf16_round(a):
    """Exact fp32 values rounded once to bf16, as float64 on a's device."""
    return from_bits16(bf16_bits(a), a.device).reshape(a.shape)


def bits16(t):
    """A bf16 tensor's bit patterns, numpy uint16, in memory order of the given (contiguous) view."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bits32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def is_tie(a):
    """Elements of an exact (integer-valued float64) tensor that sit half way between two bf16 values."""
    f = a.to(torch.float32).cpu().numpy().view(np.uint32)
    return (f & 0xFFFF) == 0x8000


def prep_images_ref(bits, cin, cout, wl):
    """(wf, wd) bf16 patterns of bb_conv3x3_prep for the weight whose fp32 patterns are ``bits`` (numpy uint32) in
    layout wl (0: w[co][ci][t], 1: w[co][t][ci]): wf[t][co][ci] and wd[8 - t][ci][co], cast by R.bf16_rne."""
    h = R.bf16_rne(np.asarray(bits, np.uint32).view(np.float32))
    w = h.reshape(cout, 9, cin).transpose(0, 2, 1) if wl else h.reshape(cout, cin, 9)  # -> [co][ci][t]
    wf = w.transpose(2, 0, 1)
    wd = w.transpose(2, 1, 0)[::-1]
    return np.ascontiguousarray(wf).reshape(-1), np.ascontiguousarray(wd).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------
# Launch geometry (bb_conv.hip: wgrad_chunks, wgrad_bpc, wgrad_used, in_wgrad_chunks, launch_conv_in_forward,
# conv3x3_stats_blocks)
# ---------------------------------------------------------------------------------------------------------------
Geometry = namedtuple("Geometry", "nchunk bpc used last")  # last: boards in the last chunk that holds any


def wgrad_geometry(nb, cin, cout):
    tiles = (cin // 64) * (cout // 64)
    nchunk = max(1, min(256 // tiles, (nb + 1) // 2))
    bpc = -(-nb // nchunk)
    bpc = (bpc + 1) // 2 * 2
    used = -(-nb // bpc)
    return Geometry(nchunk, bpc, used, nb - (used - 1) * bpc)


def wgrad_workspace_bytes(nb, cin, cout):
    return wgrad_geometry(nb, cin, cout).nchunk * 9 * cin * cout * 4


def stages(boards):
    """LDS stages (2 boards each) of a chunk of ``boards`` boards."""
    return (boards + 1) // 2


def in_wgrad_chunks(nb):
    return min(128, (nb + 3) // 4)


def in_wgrad_workspace_bytes(nb):
    return in_wgrad_chunks(nb) * 9 * 64 * 4 * 4


def in_fwd_blocks(nb):
    return min(256, (nb + 3) // 4)


def stats_blocks(nb):
    return (nb + 1) // 2


# ---------------------------------------------------------------------------------------------------------------
# Integer inputs.  Board b's values depend on (family, kind, channels, b) alone, so a batch of nb boards is the
# first nb boards of every larger batch of the same family: bounds shown on the largest batch hold on the smaller.
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("small", "wide")
W_RANGE = {"small": {64: 2, 128: 2}, "wide": {64: 20, 128: 14}}  # |w| <= W_RANGE[family][cin]
G_RANGE = {"small": 2, "wide": 3}  # |dy| <=
G_KEEP = {"small": 8, "wide": 15}  # twentieths of the dy entries kept (the rest zeroed)
_FAM_SEED = {"small": 11, "wide": 23}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_x(family, nb, cin):
    """x in {-1, 0, 1}, a quarter of the entries zeroed on top: [nb, 8, 8, cin] float64 (CPU)."""
    g = _gen(1000 * _FAM_SEED[family] + cin)
    x = torch.randint(-1, 2, (nb, 8, 8, cin), generator=g)
    keep = torch.randint(0, 4, (nb, 8, 8, cin), generator=_gen(7000 * _FAM_SEED[family] + cin)) > 0
    return (x * keep).double()


def int_w(family, cin, cout):
    r = W_RANGE[family][cin]
    g = _gen(2000 * _FAM_SEED[family] + 3 * cin + cout)
    return torch.randint(-r, r + 1, (cout, cin, 3, 3), generator=g).double()


def int_g(family, nb, cout):
    r = G_RANGE[family]
    g = _gen(3000 * _FAM_SEED[family] + cout)
    dy = torch.randint(-r, r + 1, (nb, 8, 8, cout), generator=g)
    keep = torch.randint(0, 20, (nb, 8, 8, cout), generator=_gen(9000 * _FAM_SEED[family] + cout)) < G_KEEP[family]
    return (dy * keep).double()


def one_hot_w(cin, cout):
    """Integer one-hot weights on every tap: output channel co reads tap co % 9 of input channel (5 co + 3) % cin,
    scaled 1 + co % 9 -- a reversed or transposed tap moves a value instead of changing a sum."""
    w = torch.zeros((cout, cin, 3, 3), dtype=torch.float64)
    for co in range(cout):
        t = co % 9
        w[co, (5 * co + 3) % cin, t // 3, t % 3] = 1.0 + t
    return w


BnParams = namedtuple("BnParams", "bx mean invstd weight bias")


def int_bn(nb, c, seed=5):
    """Dyadic BatchNorm-backward operands: bx integers in -4..4, mean an integer, invstd in {0.5, 1, 2}, the weight
    +-{0.5, 1, 2}, the bias an integer -- xhat, the ReLU argument and the three sums are exact in fp32."""
    g = _gen(seed + c)
    bx = torch.randint(-4, 5, (nb, 8, 8, c), generator=g).double()
    mean = torch.randint(-1, 2, (c,), generator=g).double()
    invstd = 2.0 ** torch.randint(-1, 2, (c,), generator=g).double()
    weight = 2.0 ** torch.randint(-1, 2, (c,), generator=g).double() * (1 - 2 * torch.randint(0, 2, (c,), generator=g))
    bias = torch.randint(-2, 3, (c,), generator=g).double()
    return BnParams(bx, mean, invstd, weight, bias)


def bn_backward_terms(gy, bn, relu):
    """(g, g xhat, xhat) per element, float64, from the stored gradient gy [nb, 8, 8, c]: g = gy masked where the
    forward's ReLU argument (bx - mean) (invstd weight) + bias is <= 0."""
    u = bn.bx.to(gy.device)
    mean, invstd, weight, bias = (v.to(gy.device) for v in (bn.mean, bn.invstd, bn.weight, bn.bias))
    arg = (u - mean) * (invstd * weight) + bias
    g = torch.where(arg <= 0, torch.zeros_like(gy), gy) if relu else gy
    xh = (u - mean) * invstd
    return g, g * xh, xh, arg


def per_block(a, boards=2):
    """[nb, 8, 8, c] -> [ceil(nb / boards), c]: the sum over each forward workgroup's pixels (boards past the batch
    count nothing)."""
    nb, c = a.shape[0], a.shape[3]
    nblk = -(-nb // boards)
    pad = torch.zeros((nblk * boards, c), dtype=a.dtype, device=a.device)
    pad[:nb] = a.reshape(nb, 64, c).sum(1)
    return pad.reshape(nblk, boards, c).sum(1)


# ---------------------------------------------------------------------------------------------------------------
# The catalogue
# ---------------------------------------------------------------------------------------------------------------
FWD_NB = (1, 2, 3, 5, 257)
_WGRAD_EXTRA = {
    (128, 128): (129, 130, 131, 261, 387, 577),
    (64, 128): (387, 515, 1031),
    (128, 64): (387, 515, 1031),
    (64, 64): (515, 1031, 2051, 3585),  # 3585: 8 stages (bpc 16), the one depth past the ring that 2048 does not give
}
_WGRAD_COMMON = (1, 2, 3, 5, 64, 2048)  # 1, 5, 64, 2048: the batch sizes tests/test_gpu_conv.py runs

WgradCase = namedtuple("WgradCase", "cin cout nb geo")


def wgrad_cases():
    return [WgradCase(cin, cout, nb, wgrad_geometry(nb, cin, cout))
            for cin, cout in PAIRS for nb in sorted(_WGRAD_COMMON + _WGRAD_EXTRA[(cin, cout)])]


IN_FWD_NB = (1, 3, 4, 5, 8, 9, 1023, 1024, 1025, 1029)
IN_WGRAD_NB = (1, 4, 5, 509, 512, 513, 517)


def in_case_layouts(i):
    """(x_nhwc, w_layout) of the i-th input-layer case: all four combinations, spread over the list."""
    return i & 1, (i >> 1) & 1


def int_in_x(nb, planes01, seed=41):
    """The input layer's x [nb, 8, 8, 4] float64: 0/1 board planes, or integers in -3..3."""
    g = _gen(seed + nb)
    if planes01:
        return (torch.rand((nb, 8, 8, 4), generator=g) < 0.4).double()
    return torch.randint(-3, 4, (nb, 8, 8, 4), generator=g).double()


def int_in_w(seed=43):
    return torch.randint(-8, 9, (64, 4, 3, 3), generator=_gen(seed)).double()


# ---------------------------------------------------------------------------------------------------------------
# Guarded device buffers
# ---------------------------------------------------------------------------------------------------------------
SENT = {torch.bfloat16: 0xBEEF, torch.float32: 0x7FC0BEEF, torch.float64: 0x7FF8BEEF0BADF00D}  # the last two are NaNs
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def guarded(device, dtype, n, pad):
    """(flat, view): n elements of ``dtype`` with ``pad`` guard elements on each side, every element (the view's
    included) filled with the sentinel bit pattern, a NaN for the float types.  pad keeps 16-byte alignment."""
    it = _INT[dtype]
    size = torch.empty((), dtype=dtype).element_size()
    assert pad * size % 16 == 0
    flat = torch.full((pad + n + pad,), _signed(SENT[dtype], 8 * size), dtype=it, device=device).view(dtype)
    view = flat[pad:pad + n]
    assert view.data_ptr() % 16 == 0
    return flat, view


def guards_ok(flat, n, pad, tail_from=None):
    """The guard elements still hold the sentinel; with ``tail_from`` also the view's elements from that index on."""
    b = flat.view(_INT[flat.dtype])
    s = _signed(SENT[flat.dtype], 8 * flat.element_size())
    hi = pad + (n if tail_from is None else tail_from)
    return bool((b[:pad] == s).all()) and bool((b[hi:] == s).all())


def nhwc_bf16(a, device):
    """Integer-valued [nb, 8, 8, C] float64 -> the same values as a flat bf16 device tensor (exactly)."""
    t = a.to(device).to(torch.bfloat16)
    assert bool((t.double() == a.to(device)).all()), "inputs must be exact in bf16"
    return t.contiguous().view(-1)
