"""The bf16 weight gradient (csrc/bb_conv.hip: conv_wgrad_kernel, conv_wgrad_reduce) at every depth and tail of its
stage ring, and the 4 -> 64 input layer (conv_in_fwd_kernel, conv_in_wgrad_kernel), bit for bit on integer data.

Integer cases.  tests/_conv_ref.wgrad_cases() holds, for each channel pair, batch sizes that give 1, 2, 3, 4 or 5
and 8 or more LDS stages per chunk, an odd last board at the first and at a later stage, a last chunk shorter than the
others, a chunk count that is and is not a multiple of 8 and one below the grid's (tests/test_conv_edges_cpu.py
asserts that).  With x in {-1, 0, 1} and dy in {-2 .. 2} every partial sum is an integer below 2^24, so dw must equal
the float64 restatement in every bit, through bb_conv3x3_wgrad in both weight layouts and through
bb_conv3x3_wgrad_partial + bb_conv3x3_wgrad_reduce, twice.  The workspace is prefilled with NaN: the chunks in use
must all be written, and nothing past them.

Random bf16 data: the bound.  dw[co, ci, t] is a sum of exact products (bf16 x bf16 fits fp32).  A product is added
to an MFMA accumulator that holds the earlier pixels of the same half's boards in the chunk -- waves 0-3 take the
first board of every stage and waves 4-7 the second, so one accumulator sees bpc / 2 boards x 64 pixels -- then the
second half's sum is added to the first's (1), then conv_wgrad_reduce adds the `used` chunk partials in order.
Counting every addition of a product or partial as one fp32 rounding (an MFMA that rounds less often only helps), the
longest chain has B = 32 bpc + 1 + used additions, of which the first of each accumulator and the reduction's first
(onto 0) are exact.  With u = 2^-24 the standard bound for a chain of B - 2 roundings is
gamma = (B - 2) u / (1 - (B - 2) u) <= B u (as B^2 < 2^25), so

    |dw - dw64| <= B 2^-24 sum |dy x|        per element, B = 32 bpc + 1 + used,

with dw64 and sum |dy x| from float64.  The test prints the worst ratio error / bound beside the same figure for
torch's fp32 weight gradient (not asserted).  Measured on an MI355X over the eight cases: 0.0001 to 0.0005 of the
bound, torch 0.0001 to 0.0007 -- the bound is a worst case over B roundings of one sign, the errors add like sqrt(B).
"""
import numpy as np
import pytest
import torch

import _conv_ref as CR

pytestmark = pytest.mark.gpu

_CASES = CR.wgrad_cases()
_ID = [f"{c.cin}-{c.cout}-{c.nb}" for c in _CASES]


def _dw_layout(ref, wl):
    """[cout, cin, 3, 3] -> the flat order of w_layout wl: [co][ci][t] or [co][t][ci]."""
    return (ref.permute(0, 2, 3, 1) if wl else ref).contiguous().view(-1)


class _Wgrad:
    """The guarded buffers of one (nb, cin, cout) and the library calls on them."""

    def __init__(self, lib, cuda, nb, cin, cout):
        self.lib, self.cuda, self.nb, self.cin, self.cout = lib, cuda, nb, cin, cout
        self.geo = CR.wgrad_geometry(nb, cin, cout)
        self.k = 9 * cin * cout  # floats per chunk
        assert lib.bb_conv3x3_workspace_bytes(nb, cin, cout) == 4 * self.k * self.geo.nchunk
        assert lib.bb_conv3x3_wgrad_chunks(nb, cin, cout) == self.geo.used

    def fresh(self):
        self.ws_flat, self.ws = CR.guarded(self.cuda, torch.float32, self.k * self.geo.nchunk, self.k)
        self.dw_flat, self.dw = CR.guarded(self.cuda, torch.float32, self.k, 4096)

    def whole(self, x, dy, wl):
        from runtime import kernels as K

        self.fresh()
        K.L.check(self.lib.bb_conv3x3_wgrad(K._p(x), K._p(dy), self.nb, self.cin, self.cout, K._p(self.ws), wl,
                                            K._p(self.dw), K._s(self.cuda)), "wgrad")
        return self.checked()

    def split(self, x, dy, wl):
        from runtime import kernels as K

        self.fresh()
        K.L.check(self.lib.bb_conv3x3_wgrad_partial(K._p(x), K._p(dy), self.nb, self.cin, self.cout, K._p(self.ws),
                                                    K._s(self.cuda)), "wgrad_partial")
        K.L.check(self.lib.bb_conv3x3_wgrad_reduce(K._p(self.ws), self.geo.used, self.cin, self.cout, wl,
                                                   K._p(self.dw), K._s(self.cuda)), "wgrad_reduce")
        return self.checked()

    def checked(self):
        used = self.geo.used * self.k
        assert not bool(torch.isnan(self.ws[:used]).any()), "a chunk in use was not written completely"
        assert CR.guards_ok(self.ws_flat, self.ws.numel(), self.k, tail_from=used), "a store past the chunks in use"
        assert CR.guards_ok(self.dw_flat, self.k, 4096), "a store outside dw"
        return self.dw.clone()


def _same_bits(got, ref64, what):
    want = ref64.to(torch.float32)
    assert bool((want.double() == ref64).all())
    g, w = CR.bits32(got), CR.bits32(want)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} weights differ, first at {bad[:5]}"


@pytest.mark.parametrize("case", _CASES, ids=_ID)
def test_weight_gradient_bit_exact(cuda, lib, case):
    cin, cout, nb = case.cin, case.cout, case.nb
    x64, g64 = CR.int_x("small", nb, cin).to(cuda), CR.int_g("small", nb, cout).to(cuda)
    ref = CR.conv_wgrad(x64, g64)
    x, dy = x64.to(torch.bfloat16).view(-1), g64.to(torch.bfloat16).view(-1)
    del x64, g64
    run = _Wgrad(lib, cuda, nb, cin, cout)
    first = run.whole(x, dy, 0)
    _same_bits(first, _dw_layout(ref, 0), "bb_conv3x3_wgrad, layout 0")
    _same_bits(run.whole(x, dy, 1), _dw_layout(ref, 1), "bb_conv3x3_wgrad, layout 1")
    _same_bits(run.split(x, dy, nb % 2), _dw_layout(ref, nb % 2), "wgrad_partial + wgrad_reduce")
    assert torch.equal(run.whole(x, dy, 0).view(torch.int32), first.view(torch.int32)), "a second call differs"


def _deep_case(cin, cout):
    """The pair's catalogue case with 5 stages per chunk (the ring wraps) and the most chunks."""
    return max((c for c in _CASES if (c.cin, c.cout) == (cin, cout) and c.geo.bpc == 10), key=lambda c: c.nb)


@pytest.mark.parametrize("where", ["first", "middle", "last", "batch_last"])
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_single_board_reveals_the_chunk_walk(cuda, lib, cin, cout, where):
    """dy and x zero except in one board, where x = 1 and dy = 1 + co % 3: every weight is then that board's count
    of pixels under the tap times 1 + co % 3, nonzero everywhere, so a board the kernel skips zeroes every weight
    and one it takes twice doubles every weight."""
    case = _deep_case(cin, cout)
    nb, bpc = case.nb, case.geo.bpc
    board = {"first": bpc, "middle": bpc + bpc // 2, "last": 2 * bpc - 1, "batch_last": nb - 1}[where]
    if where == "batch_last":
        assert case.geo.last % 2 == 1  # an odd board: alone in its stage
    x = torch.zeros((nb, 8, 8, cin), dtype=torch.bfloat16, device=cuda)
    dy = torch.zeros((nb, 8, 8, cout), dtype=torch.bfloat16, device=cuda)
    x[board] = 1.0
    dy[board] = (1 + torch.arange(cout, device=cuda) % 3).to(torch.bfloat16)
    ref = CR.conv_wgrad(x[board:board + 1], dy[board:board + 1])
    assert float(ref.abs().min()) >= 49
    run = _Wgrad(lib, cuda, nb, cin, cout)
    _same_bits(run.whole(x.view(-1), dy.view(-1), 0), _dw_layout(ref, 0), f"one board ({where})")


def _random_inputs(cuda, n, cin, cout, seed):
    """tests/test_gpu_conv.py's generator: standard normal bf16 activations and gradients (channels_last)."""
    g = torch.Generator(device=cuda).manual_seed(seed)
    x = torch.randn((n, cin, 8, 8), device=cuda, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    torch.randn((cout, cin, 3, 3), device=cuda, generator=g)  # the weight draw of that generator (not used here)
    dy = torch.randn((n, cout, 8, 8), device=cuda, generator=g).bfloat16().contiguous(
        memory_format=torch.channels_last)
    return x, dy


def _random_nbs():
    out = []
    for cin, cout in CR.PAIRS:
        largest = max(c.nb for c in _CASES if (c.cin, c.cout) == (cin, cout) and c.nb != 2048)
        out += [(cin, cout, largest), (cin, cout, 2048)]
    return out


@pytest.mark.parametrize("cin,cout,nb", _random_nbs())
def test_random_data_within_the_summation_bound(cuda, lib, cin, cout, nb):
    xc, dyc = _random_inputs(cuda, nb, cin, cout, 7 * nb + cin - cout)
    x, dy = xc.permute(0, 2, 3, 1), dyc.permute(0, 2, 3, 1)  # NHWC views of the channels_last storage
    assert x.is_contiguous() and dy.is_contiguous()
    ref = CR.conv_wgrad(x, dy)
    mag = CR.conv_wgrad(x, dy, absolute=True)
    geo = CR.wgrad_geometry(nb, cin, cout)
    B = 32 * geo.bpc + 1 + geo.used
    bound = B * 2.0 ** -24 * mag
    run = _Wgrad(lib, cuda, nb, cin, cout)
    got = run.whole(x.reshape(-1), dy.reshape(-1), 0).view(cout, cin, 3, 3).double()
    ours = float(((got - ref).abs() / bound).max())
    tw = torch.nn.grad.conv2d_weight(xc.float(), (cout, cin, 3, 3), dyc.float(), padding=1).double()
    theirs = float(((tw - ref).abs() / bound).max())
    print(f"\nwgrad {cin}->{cout} nb {nb}: bpc {geo.bpc} used {geo.used} B {B}; worst error / bound: "
          f"bb_conv3x3_wgrad {ours:.4f}, torch fp32 conv2d_weight {theirs:.4f}")
    assert ours <= 1.0, ours


# ---------------------------------------------------------------------------------------------------------------
# The input layer
# ---------------------------------------------------------------------------------------------------------------
def _in_operands(cuda, x64, w64, x_nhwc, wl):
    x = (x64 if x_nhwc else x64.permute(0, 3, 1, 2)).contiguous().to(cuda).float().view(-1)
    w = (w64.permute(0, 2, 3, 1) if wl else w64).contiguous().to(cuda).float().view(-1)
    return x, w


def _in_out(cuda, nb):
    pad = 4 * 64 * 64  # four boards of output rows on each side
    flat, view = CR.guarded(cuda, torch.bfloat16, nb * 64 * 64, pad)
    return flat, view, pad


@pytest.mark.parametrize("planes01", [1, 0])
@pytest.mark.parametrize("i", range(len(CR.IN_FWD_NB)), ids=[str(n) for n in CR.IN_FWD_NB])
def test_conv_in_forward_bit_exact(cuda, lib, i, planes01):
    from runtime import kernels as K

    nb = CR.IN_FWD_NB[i]
    x_nhwc, wl = CR.in_case_layouts(i + planes01)
    x64, w64 = CR.int_in_x(nb, planes01), CR.int_in_w()
    x, w = _in_operands(cuda, x64, w64, x_nhwc, wl)
    flat, view, pad = _in_out(cuda, nb)
    K.L.check(lib.bb_conv_in_forward(K._p(x), x_nhwc, K._p(w), wl, nb, K._p(view), K._s(cuda)), "conv_in_forward")
    want = CR.bf16_bits(CR.conv_forward(x64.to(cuda), w64.to(cuda))).reshape(-1)
    got = CR.bits16(view)
    assert np.array_equal(got, want), f"{int((got != want).sum())} elements differ"
    assert CR.guards_ok(flat, view.numel(), pad), "a store outside y"


@pytest.mark.parametrize("i", range(len(CR.IN_WGRAD_NB)), ids=[str(n) for n in CR.IN_WGRAD_NB])
def test_conv_in_weight_gradient_bit_exact(cuda, lib, i):
    from runtime import kernels as K

    nb = CR.IN_WGRAD_NB[i]
    x_nhwc, _ = CR.in_case_layouts(i)
    x64, g64 = CR.int_in_x(nb, planes01=i % 3 == 0), CR.int_g("wide", nb, 64)
    x, _ = _in_operands(cuda, x64, CR.int_in_w(), x_nhwc, 0)
    dy = CR.nhwc_bf16(g64, cuda)
    ref = CR.conv_wgrad(x64.to(cuda), g64.to(cuda))
    chunks = CR.in_wgrad_chunks(nb)
    k = 9 * 64 * 4
    assert lib.bb_conv_in_wgrad_workspace_bytes(nb) == 4 * k * chunks
    for wl in (0, 1):
        ws_flat, ws = CR.guarded(cuda, torch.float32, k * chunks, k)
        dw_flat, dw = CR.guarded(cuda, torch.float32, k, 4096)
        K.L.check(lib.bb_conv_in_wgrad(K._p(x), x_nhwc, K._p(dy), nb, K._p(ws), wl, K._p(dw), K._s(cuda)),
                  "conv_in_wgrad")
        assert not bool(torch.isnan(ws).any()), "a workgroup's partial was not written completely"
        assert CR.guards_ok(ws_flat, ws.numel(), k) and CR.guards_ok(dw_flat, k, 4096)
        _same_bits(dw, _dw_layout(ref, wl), f"conv_in_wgrad, layout {wl}")


@pytest.mark.parametrize("nb", [1, 1025])
def test_conv_in_forward_prep_is_both_calls(cuda, lib, nb):
    """bb_conv_in_forward_prep: y of bb_conv_in_forward and the images of bb_conv3x3_prep_multi, in one launch
    (1 and 256 forward workgroups ahead of the prep workgroups)."""
    import ctypes as C

    from runtime import kernels as K

    x64, w64 = CR.int_in_x(nb, planes01=1), CR.int_in_w()
    x, w = _in_operands(cuda, x64, w64, nb % 2, 1)
    layers = [(64, 128, 0), (128, 128, 1), (128, 64, 1), (64, 64, 0)]
    gen = torch.Generator(device=cuda).manual_seed(nb)
    ws = [torch.randn(9 * ci * co, device=cuda, generator=gen) for ci, co, _ in layers]
    ints = [(C.c_int32 * len(layers))(*[l[j] for l in layers]) for j in range(3)]

    def images():
        bufs = [[CR.guarded(cuda, torch.bfloat16, 9 * ci * co, 1024) for ci, co, _ in layers] for _ in range(2)]
        return bufs, [K._ptrs([b[1] for b in side]) for side in bufs]

    (yflat, y, pad), plain = _in_out(cuda, nb), _in_out(cuda, nb)
    bufs, (wf, wd) = images()
    K.L.check(lib.bb_conv_in_forward_prep(K._p(x), nb % 2, K._p(w), 1, nb, K._p(y), len(layers), K._ptrs(ws), *ints,
                                          wf, wd, K._s(cuda)), "conv_in_forward_prep")
    K.L.check(lib.bb_conv_in_forward(K._p(x), nb % 2, K._p(w), 1, nb, K._p(plain[1]), K._s(cuda)), "conv_in_forward")
    rbufs, (rwf, rwd) = images()
    K.L.check(lib.bb_conv3x3_prep_multi(len(layers), K._ptrs(ws), *ints, rwf, rwd, K._s(cuda)), "prep_multi")
    assert torch.equal(y.view(torch.int16), plain[1].view(torch.int16)) and CR.guards_ok(yflat, y.numel(), pad)
    assert np.array_equal(CR.bits16(y), CR.bf16_bits(CR.conv_forward(x64.to(cuda), w64.to(cuda))).reshape(-1))
    for side, rside in zip(bufs, rbufs):
        for (flat, img), (rflat, rimg) in zip(side, rside):
            assert torch.equal(img.view(torch.int16), rimg.view(torch.int16))
            assert CR.guards_ok(flat, img.numel(), 1024) and CR.guards_ok(rflat, rimg.numel(), 1024)
