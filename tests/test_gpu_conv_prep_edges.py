"""The f32 -> bf16 weight images of bb_conv3x3_prep and bb_conv3x3_prep_multi (csrc/bb_conv.hip, conv_prep_kernel and
prep_block), pinned directly.

Layout, from the kernel's comment and its two stores: the forward image is wf[t][co][ci] and the data-gradient image
wd[8 - t][ci][co], plain row-major, of w[co][ci][t] (w_layout 0) or w[co][t][ci] (w_layout 1).  The images in memory
are not swizzled: the XOR keys in bb_conv.hip (wkey, fwd_key) permute the *source* addresses of the global -> LDS
copies in conv_fwd_kernel's stage_w, so only the LDS copy is swizzled.  The cast is round to nearest even, restated on
the bit patterns by tests/_optim_ref.bf16_rne: ties with an even and an odd kept mantissa, values that round up into
the next binade, +-0, fp32 subnormals, the largest finite value (-> Inf), +-Inf and NaN (stays NaN; payload free).

bb_conv3x3_prep_multi packs the layers' workgroups back to back (block0).  Every layer here has 9 cin cout elements, a
multiple of 256 for channels of 64 and 128, so no layer's last workgroup is partly idle and the `i >= cout cin 9`
return is never taken with these shapes; the whole images are compared, which includes the elements on each side of
every block0 boundary.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _conv_ref as CR
import _optim_ref as R

pytestmark = pytest.mark.gpu

PAD = 1024
# fp32 patterns placed at the head of every weight: ties on an even kept mantissa (round down) and an odd one (round
# up), either sign; a tie and a near-tie that carry into the next binade; +-0; subnormals (and their tie); the largest
# finite value and the last tie below infinity; +-Inf; quiet and signalling NaNs
SPECIAL = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3FFF8000, 0x3FFFC000,
                    0xBFFF8000, 0x407F8000, 0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,
                    0x007F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000,
                    0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7F80FFFF, 0x7FFFFFFF], dtype=np.uint32)


def _weight_bits(n, seed):
    """n fp32 patterns: SPECIAL, then draws from the cast tests' value set (every bf16 pattern, its fp32 neighbours
    and its tie), NaNs included."""
    rng = np.random.default_rng(seed)
    pats = R.cast_patterns()
    bits = pats[rng.integers(0, pats.size, n)]
    bits[:SPECIAL.size] = SPECIAL
    return bits


def _device_f32(cuda, bits):
    return torch.from_numpy(bits.view(np.int32).copy()).to(cuda).view(torch.float32)


def _image(cuda, n):
    return CR.guarded(cuda, torch.bfloat16, n, PAD)


def _prep(lib, cuda, w, cin, cout, wl):
    from runtime import kernels as K

    n = 9 * cin * cout
    (ff, wf), (df, wd) = _image(cuda, n), _image(cuda, n)
    K.L.check(lib.bb_conv3x3_prep(K._p(w), cin, cout, wl, K._p(wf), K._p(wd), K._s(cuda)), "prep")
    assert CR.guards_ok(ff, n, PAD) and CR.guards_ok(df, n, PAD), "a store outside an image"
    return wf, wd


def _same_or_both_nan(got, want, what):
    nan = R.is_nan_bf16(want)
    assert np.array_equal(R.is_nan_bf16(got), nan), f"{what}: NaNs differ"
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at {bad[:5]}: got {got[bad[:5]]}, "
                           f"want {want[bad[:5]]}")


@pytest.mark.parametrize("wl", [0, 1])
@pytest.mark.parametrize("cin,cout", CR.PAIRS)
def test_prep_images_are_the_nearest_even_cast_of_the_permuted_weight(cuda, lib, cin, cout, wl):
    bits = _weight_bits(9 * cin * cout, 31 * cin + cout + wl)
    want_f, want_d = CR.prep_images_ref(bits, cin, cout, wl)
    assert int(R.is_nan_bf16(want_f).sum()) >= 5 and int((want_f == 0x7F80).sum()) >= 2  # NaN stays, overflow -> Inf
    wf, wd = _prep(lib, cuda, _device_f32(cuda, bits), cin, cout, wl)
    _same_or_both_nan(CR.bits16(wf), want_f, "wf[t][co][ci]")
    _same_or_both_nan(CR.bits16(wd), want_d, "wd[8-t][ci][co]")


_MIXED = [(64, 128, 0), (128, 128, 1), (128, 64, 1), (64, 64, 0), (128, 128, 0), (64, 128, 1), (64, 64, 1),
          (128, 64, 0)]


@pytest.mark.parametrize("count", [1, 2, 16])
def test_prep_multi_is_per_layer_prep(cuda, lib, count):
    from runtime import kernels as K

    layers = [_MIXED[(l + count) % len(_MIXED)] for l in range(count)]
    ws = [_device_f32(cuda, _weight_bits(9 * ci * co, 100 * count + l)) for l, (ci, co, _) in enumerate(layers)]
    bufs = [[_image(cuda, 9 * ci * co) for ci, co, _ in layers] for _ in range(2)]
    ints = [(C.c_int32 * count)(*[l[j] for l in layers]) for j in range(3)]
    K.L.check(lib.bb_conv3x3_prep_multi(count, K._ptrs(ws), *ints, K._ptrs([b[1] for b in bufs[0]]),
                                        K._ptrs([b[1] for b in bufs[1]]), K._s(cuda)), "prep_multi")
    assert sum(9 * ci * co // 256 for ci, co, _ in layers) * 256 == sum(9 * ci * co for ci, co, _ in layers)
    for l, (ci, co, wl) in enumerate(layers):
        wf, wd = _prep(lib, cuda, ws[l], ci, co, wl)
        for side, single in ((0, wf), (1, wd)):
            flat, img = bufs[side][l]
            assert CR.guards_ok(flat, img.numel(), PAD), f"layer {l}: a store outside image {side}"
            assert np.array_equal(CR.bits16(img), CR.bits16(single)), f"layer {l} image {side}"
        want_f, want_d = CR.prep_images_ref(CR.bits32(ws[l]), ci, co, wl)
        _same_or_both_nan(CR.bits16(bufs[0][l][1]), want_f, f"layer {l} wf")
        _same_or_both_nan(CR.bits16(bufs[1][l][1]), want_d, f"layer {l} wd")
