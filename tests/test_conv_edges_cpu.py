"""tests/_conv_ref.py checked on the host, and the convolution entry points' refusals.

The float64 restatement of the 3x3 / pad-1 convolution against torch's float64 conv2d / conv2d_input / conv2d_weight;
the Python launch geometry against the library's host queries; that the weight-gradient catalogue reaches every
depth and tail of conv_wgrad_kernel's stage ring; that the integer families are fair to fp32 (every partial sum the
kernels can form is exact, so the GPU tests may ask for bit equality); and that every convolution entry point refuses
bad arguments on the host, before any launch (no GPU is needed: a refused call reaches no HIP call).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as CR

BB_ERR_ARG = -1


def _nchw(a):
    return a.permute(0, 3, 1, 2).contiguous()


def _nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("nb,cin,cout", [(1, 64, 64), (3, 64, 128), (2, 128, 64), (3, 128, 128), (3, 4, 64)])
@pytest.mark.parametrize("integer", [True, False])
def test_reference_is_torch_float64(nb, cin, cout, integer):
    g = torch.Generator().manual_seed(nb + cin + 2 * cout)
    if integer:
        x = torch.randint(-3, 4, (nb, 8, 8, cin), generator=g).double()
        w = torch.randint(-9, 10, (cout, cin, 3, 3), generator=g).double()
        dy = torch.randint(-3, 4, (nb, 8, 8, cout), generator=g).double()
    else:
        x = torch.randn((nb, 8, 8, cin), generator=g, dtype=torch.float64)
        w = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64)
        dy = torch.randn((nb, 8, 8, cout), generator=g, dtype=torch.float64)
    pairs = [
        (CR.conv_forward(x, w), _nhwc(F.conv2d(_nchw(x), w, padding=1))),
        (CR.conv_dgrad(dy, w), _nhwc(torch.nn.grad.conv2d_input((nb, cin, 8, 8), w, _nchw(dy), padding=1))),
        (CR.conv_wgrad(x, dy), torch.nn.grad.conv2d_weight(_nchw(x), w.shape, _nchw(dy), padding=1)),
    ]
    for got, ref in pairs:
        assert got.dtype == torch.float64 and got.shape == ref.shape
        if integer:
            assert torch.equal(got, ref)
        else:
            assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))
    assert torch.equal(CR.conv_wgrad(x, dy, absolute=True), CR.conv_wgrad(x.abs(), dy.abs()))


def test_bf16_rounding_helpers():
    a = torch.tensor([0.0, 1.0, 255.0, 256.0, 257.0, 258.0, 259.0, 511.0, 513.0, 514.0, -257.0, -259.0]).double()
    want = torch.tensor([0.0, 1.0, 255.0, 256.0, 256.0, 258.0, 260.0, 512.0, 512.0, 512.0, -256.0, -260.0]).double()
    assert torch.equal(CR.bf16_round(a), want)
    assert CR.is_tie(a).tolist() == [False, False, False, False, True, False, True, True, False, True, True, True]
    assert torch.equal(CR.bf16_round(a), a.bfloat16().double())  # torch's CPU cast is the same rounding
    with pytest.raises(AssertionError):
        CR.bf16_bits(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64))


def test_prep_image_reference_layout():
    """Element (co, ci, t) of the weight lands at wf[t][co][ci] and wd[8 - t][ci][co], from either layout: weights
    whose value is their co, their ci and their t in turn."""
    cin, cout = 64, 128
    idx = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(9), indexing="ij")
    for which in range(3):
        val = idx[which].astype(np.float32)  # at most 127: exact in bf16
        for wl in (0, 1):
            src = np.ascontiguousarray(val.transpose(0, 2, 1) if wl else val).reshape(-1).view(np.uint32)
            wf, wd = (CR.from_bits16(h).numpy() for h in CR.prep_images_ref(src, cin, cout, wl))
            assert np.array_equal(wf.reshape(9, cout, cin), val.transpose(2, 0, 1))
            assert np.array_equal(wd.reshape(9, cin, cout)[::-1], val.transpose(2, 1, 0))


def test_geometry_is_the_librarys(lib):
    nbs = list(range(1, 4201)) + [65536, 100000]
    bad = []
    for cin, cout in CR.PAIRS:
        for nb in nbs:
            geo = CR.wgrad_geometry(nb, cin, cout)
            got = (lib.bb_conv3x3_wgrad_chunks(nb, cin, cout), lib.bb_conv3x3_workspace_bytes(nb, cin, cout),
                   lib.bb_conv3x3_stats_blocks(nb, cout))
            want = (geo.used, CR.wgrad_workspace_bytes(nb, cin, cout), CR.stats_blocks(nb))
            if got != want:
                bad.append((cin, cout, nb, got, want))
            assert geo.bpc % 2 == 0 and 1 <= geo.used <= geo.nchunk and 1 <= geo.last <= geo.bpc
            assert (geo.used - 1) * geo.bpc + geo.last == nb
    for nb in nbs:
        if lib.bb_conv_in_wgrad_workspace_bytes(nb) != CR.in_wgrad_workspace_bytes(nb):
            bad.append(("in", nb))
    assert not bad, bad[:10]


@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_catalogue_reaches_every_depth_and_tail(cin, cout):
    cases = [c for c in CR.wgrad_cases() if (c.cin, c.cout) == (cin, cout)]
    for nb in (1, 5, 64, 2048):  # the batch sizes of tests/test_gpu_conv.py stay
        assert any(c.nb == nb for c in cases)
    depth = {CR.stages(c.geo.bpc) if c.geo.used > 1 else CR.stages(c.geo.last) for c in cases}
    assert {1, 2, 3} <= depth and depth & {4, 5} and max(depth) >= 8, depth
    assert 5 in depth  # the first wrap of the ring of 4
    odd_last = {(c.geo.last - 1) // 2 for c in cases if c.geo.last % 2}  # the stage that holds the odd last board
    assert 0 in odd_last and max(odd_last) > 0, odd_last
    assert any(c.geo.used > 1 and CR.stages(c.geo.last) < CR.stages(c.geo.bpc) for c in cases)
    assert any(c.geo.used % 8 == 0 for c in cases) and any(c.geo.used % 8 for c in cases)
    assert any(c.geo.used < c.geo.nchunk for c in cases)
    for c in cases:
        assert c.geo == CR.wgrad_geometry(c.nb, cin, cout)


def test_input_layer_catalogue():
    blocks = {nb: CR.in_fwd_blocks(nb) for nb in CR.IN_FWD_NB}
    assert blocks[1023] == blocks[1024] == 256 and blocks[1025] == 256  # 1025: the first wave takes a second board
    assert any(nb % 4 for nb in CR.IN_FWD_NB) and any(nb % 4 == 0 for nb in CR.IN_FWD_NB)
    chunks = {nb: CR.in_wgrad_chunks(nb) for nb in CR.IN_WGRAD_NB}
    assert chunks[509] == 128 and chunks[5] == 2 and chunks[513] == 128 and 513 > 4 * 128  # cap, then a second pass
    for nbs in (CR.IN_FWD_NB, CR.IN_WGRAD_NB):
        assert {CR.in_case_layouts(i) for i in range(len(nbs))} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_families_are_fair_to_fp32(cin, cout):
    """Forward and data gradient at the largest forward batch (smaller ones are its first boards): every sum of
    magnitudes below 2^24; small: every output exact in bf16; wide: a tenth of the outputs past 256, ties present."""
    nb = max(CR.FWD_NB)
    ties = 0
    for fam in CR.FAMILIES:
        x, w, g = CR.int_x(fam, nb, cin), CR.int_w(fam, cin, cout), CR.int_g(fam, nb, cout)
        assert torch.equal(CR.int_x(fam, 3, cin), x[:3]) and torch.equal(CR.int_g(fam, 3, cout), g[:3])
        zero = float((x == 0).double().mean())
        assert 0.45 < zero < 0.55 and float(x.abs().max()) == 1  # a third zero, a quarter of the rest zeroed
        for name, out, mag in (("forward", CR.conv_forward(x, w), CR.conv_forward(x.abs(), w.abs())),
                               ("dgrad", CR.conv_dgrad(g, w), CR.conv_dgrad(g.abs(), w.abs()))):
            assert float(mag.max()) < CR.F32_EXACT
            r = CR.bf16_round(out)
            # per channel and workgroup of 2 boards: the statistics' sums, over the stored values (the sum of
            # squares is formed in the forward only; the data gradient's sums are checked below)
            s1, s2 = CR.per_block(r.abs()), CR.per_block(r * r)
            assert float(s1.max()) < CR.F32_EXACT, (fam, name, float(s1.max()))
            assert name == "dgrad" or float(s2.max()) < CR.F32_EXACT, (fam, name, float(s2.max()))
            big = float((out.abs() > 256).double().mean())
            print(f"{cin}->{cout} {fam} {name}: max |out| {float(out.abs().max()):.0f}, share past 256 {big:.3f}, "
                  f"largest sum of squares {float(s2.max()):.0f}, ties {int(CR.is_tie(out).sum())}")
            if fam == "small":
                assert torch.equal(r, out), f"{name}: an output is not exact in bf16"
            else:
                assert big >= 0.10, (name, big)
                ties += int(CR.is_tie(out).sum())
            if name == "dgrad":
                # the BatchNorm-backward sums over the stored gradient: multiples of 1/2, exact below 2^23
                bn = CR.int_bn(nb, cin)
                for relu in (0, 1):
                    t0, t1, t2, arg = CR.bn_backward_terms(r, bn, relu)
                    for t in (t0, t1, t2):
                        assert bool((2 * t == (2 * t).round()).all())
                        assert float(CR.per_block(t.abs()).max()) < CR.F32_EXACT / 2
                    assert float((arg == 0).double().mean()) > 0.01  # ReLU arguments of exactly 0 are there
    assert ties >= 1000, ties


def test_weight_gradient_cases_are_fair_to_fp32():
    """sum |dy x| per weight <= 64 nb max|dy| max|x| -- a bound on every partial sum, whatever the order."""
    for c in CR.wgrad_cases():
        for fam in CR.FAMILIES:
            assert 64 * c.nb * CR.G_RANGE[fam] * 1 < CR.F32_EXACT, c
    for nb in CR.IN_WGRAD_NB:
        assert 64 * nb * 3 * 3 < CR.F32_EXACT
    x, g = CR.int_x("small", 64, 128), CR.int_g("small", 64, 128)
    assert float(CR.conv_wgrad(x, g, absolute=True).max()) <= 64 * 64 * 2
    assert 9 * 4 * 3 * 8 < CR.F32_EXACT  # the input layer's forward sums (|x| <= 3, |w| <= 8)


# ---------------------------------------------------------------------------------------------------------------
# Refusals: decided on the host before any launch.  Pointers are made-up addresses; no refused call reads one.
# ---------------------------------------------------------------------------------------------------------------
def _addr(i):
    return 0x7F0000100000 + 0x10000 * i


# name -> (argument names in order, NULL-checked pointers, 16-byte-checked pointers)
_ENTRY = {
    "bb_conv3x3_prep": ("w cin cout wl wf wd", "w wf wd", "wf wd"),
    "bb_conv3x3_forward": ("x w N cin cout y", "x w y", "x w y"),
    "bb_conv3x3_forward_add": ("x w N cin cout add y", "x w add y", "x w add y"),
    "bb_conv3x3_forward_stats": ("x w N cin cout y part", "x w y part", "x w y"),
    "bb_conv3x3_forward_bstats": ("x w N cin cout y bx mean invstd bw bb relu part",
                                  "x w y bx mean invstd bw bb part", "x w y bx"),
    "bb_conv3x3_wgrad": ("x dy N cin cout ws wl dw", "x dy ws dw", "x dy"),
    "bb_conv3x3_wgrad_partial": ("x dy N cin cout ws", "x dy ws", "x dy"),
    "bb_conv3x3_wgrad_reduce": ("ws chunks cin cout wl dw", "ws dw", ""),
}
_INTS = {"N": 4, "cin": 64, "cout": 128, "wl": 0, "relu": 1, "chunks": 2}


def _call(lib, name, **over):
    names, _, _ = _ENTRY[name]
    args = []
    for i, a in enumerate(names.split()):
        v = over.get(a, _INTS[a] if a in _INTS else _addr(i))
        args.append(v if a in _INTS else (C.c_void_p(v) if v else None))
    return getattr(lib, name)(*args, None)


@pytest.mark.parametrize("name", sorted(_ENTRY))
def test_conv3x3_entry_points_refuse_on_the_host(lib, name):
    names, ptrs, aligned = (s.split() for s in _ENTRY[name])
    bad = []
    if "N" in names:
        bad += [{"N": 0}, {"N": -3}]
    if "chunks" in names:
        bad += [{"chunks": 0}, {"chunks": -1}]
    bad += [{"cin": 32}, {"cin": 256}, {"cout": 32}, {"cout": 256}]
    if "wl" in names:
        bad += [{"wl": 2}, {"wl": -1}]
    bad += [{p: 0} for p in ptrs]
    bad += [{p: _addr(20) + off} for p in aligned for off in (2, 8)]
    for over in bad:
        assert _call(lib, name, **over) == BB_ERR_ARG, (name, over)


def test_conv3x3_size_queries_refuse(lib):
    for n, cin, cout in ((0, 64, 64), (-1, 128, 128), (4, 32, 64), (4, 64, 256), (4, 256, 64), (4, 64, 32)):
        assert lib.bb_conv3x3_workspace_bytes(n, cin, cout) == -1
        assert lib.bb_conv3x3_wgrad_chunks(n, cin, cout) == -1
    for n, cout in ((0, 64), (-5, 128), (4, 32), (4, 256)):
        assert lib.bb_conv3x3_stats_blocks(n, cout) == -1
    assert lib.bb_conv_in_wgrad_workspace_bytes(0) == -1 and lib.bb_conv_in_wgrad_workspace_bytes(-2) == -1


def _p(v):
    return C.c_void_p(v) if v else None


def test_conv_in_entry_points_refuse_on_the_host(lib):
    x, w, y, dy, ws, dw = (_addr(i) for i in range(6))

    def fwd(x=x, w=w, wl=0, n=4, y=y):
        return lib.bb_conv_in_forward(_p(x), 0, _p(w), wl, n, _p(y), None)

    def wg(x=x, dy=dy, n=4, ws=ws, wl=1, dw=dw):
        return lib.bb_conv_in_wgrad(_p(x), 1, _p(dy), n, _p(ws), wl, _p(dw), None)

    for over in ({"n": 0}, {"n": -1}, {"x": 0}, {"w": 0}, {"y": 0}, {"wl": 2}, {"wl": -1}, {"x": x + 4}, {"x": x + 8},
                 {"y": y + 2}, {"y": y + 8}):
        assert fwd(**over) == BB_ERR_ARG, over
    for over in ({"n": 0}, {"n": -1}, {"x": 0}, {"dy": 0}, {"ws": 0}, {"dw": 0}, {"wl": 2}, {"wl": -1}, {"x": x + 4},
                 {"dy": dy + 2}, {"dy": dy + 8}):
        assert wg(**over) == BB_ERR_ARG, over


def _table(count, cin=None, cout=None, wl=None, w=None, wf=None, wd=None):
    """ctypes arrays of a prep table of ``count`` layers (at least one slot, so that a count of 0 still has
    arrays to point at), every layer 64 -> 128 / layout 0 unless overridden per layer through the dicts."""
    n = max(count, 1)
    pick = lambda d, l, v: v if d is None or l not in d else d[l]  # noqa: E731
    arr = lambda vals: (C.c_void_p * n)(*vals)  # noqa: E731
    return (arr([pick(w, l, _addr(3 * l)) for l in range(n)]),
            (C.c_int32 * n)(*[pick(cin, l, 64) for l in range(n)]),
            (C.c_int32 * n)(*[pick(cout, l, 128) for l in range(n)]),
            (C.c_int32 * n)(*[pick(wl, l, 0) for l in range(n)]),
            arr([pick(wf, l, _addr(3 * l + 1)) for l in range(n)]),
            arr([pick(wd, l, _addr(3 * l + 2)) for l in range(n)]))


_BAD_TABLES = [(0, {}), (17, {}), (-1, {}), (2, {"cin": {1: 32}}), (2, {"cout": {0: 256}}), (3, {"wl": {2: 2}}),
               (2, {"w": {1: None}}), (2, {"wf": {0: None}}), (2, {"wd": {1: None}}), (2, {"wf": {1: _addr(90) + 8}}),
               (16, {"cin": {15: 4}})]


@pytest.mark.parametrize("count,over", _BAD_TABLES)
def test_prep_tables_refuse_on_the_host(lib, count, over):
    w, cin, cout, wl, wf, wd = _table(count, **over)
    assert lib.bb_conv3x3_prep_multi(count, w, cin, cout, wl, wf, wd, None) == BB_ERR_ARG
    x, w0, y = _addr(100), _addr(101), _addr(102)
    if over.get("wf", {}).get(1) == _addr(90) + 8:
        return  # bb_conv_in_forward_prep leaves the images' alignment to the table's owner
    assert lib.bb_conv_in_forward_prep(_p(x), 0, _p(w0), 0, 4, _p(y), count, w, cin, cout, wl, wf, wd,
                                       None) == BB_ERR_ARG


def test_conv_in_forward_prep_refuses_its_own_arguments(lib):
    w, cin, cout, wl, wf, wd = _table(2)
    x, w0, y = _addr(100), _addr(101), _addr(102)

    def call(x=x, w0=w0, wl0=0, n=4, y=y, tab=(w, cin, cout, wl, wf, wd)):
        return lib.bb_conv_in_forward_prep(_p(x), 0, _p(w0), wl0, n, _p(y), 2, *tab, None)

    for over in ({"n": 0}, {"x": 0}, {"w0": 0}, {"y": 0}, {"wl0": 2}, {"x": x + 8}, {"y": y + 8},
                 {"tab": (None, cin, cout, wl, wf, wd)}, {"tab": (w, cin, cout, wl, wf, None)}):
        assert call(**over) == BB_ERR_ARG, over
