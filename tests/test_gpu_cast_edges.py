"""bb_cast_multi (csrc/bb_optim.hip) at its edges: exact values and every layout path.

Direction 0 (f32 -> bf16) equals tests/_optim_ref.bf16_rne bit for bit (NaN as "is NaN") on every bf16 pattern
widened, one fp32 ulp either side of each, every tie (a pattern plus half a bf16 step, on even and odd mantissas),
fp32 subnormals, the largest finite fp32 (-> infinity), +-0, +-inf, quiet and signalling NaNs.  Direction 1 is a
shift: the fp32 bits are pattern << 16 for all 65,536 patterns, NaN payloads included.  Layouts: sizes around the
8-element vector and the 8,192-element chunk, source and destination misaligned alone and together (the scalar
branch as whole chunks), 48 tensors in one launch, permuted rows; guard elements around every destination keep their
sentinel.  And launch_cast_multi's refusal rules.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 8191, 8192, 8193, 16389)
PAD = 8  # guard elements either side of a view: 8 f32 or 8 bf16 keep the view's 16-byte phase
SENT32, SENT16 = 0xC0DEC0DE, 0xBEEF
NP_DT = {torch.float32: np.uint32, torch.bfloat16: np.uint16}
INT_DT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _buffer(cuda, dtype, n, off, bits=None):
    """A flat device buffer of sentinel bits with a view of n elements at element offset ``off`` past a 16-byte
    boundary (filled with ``bits`` when given) -> (flat, view)."""
    host = np.full(PAD + off + n + PAD, SENT32 if dtype == torch.float32 else SENT16, NP_DT[dtype])
    if bits is not None:
        host[PAD + off:PAD + off + n] = bits
    flat = torch.from_numpy(host.view(np.int32 if dtype == torch.float32 else np.int16)).to(cuda).view(dtype)
    view = flat[PAD + off:PAD + off + n]
    assert view.data_ptr() % 16 == (off * flat.element_size()) % 16
    return flat, view


def _bits(t):
    return t.view(INT_DT[t.dtype]).cpu().numpy().view(NP_DT[t.dtype])


def _guards_ok(flat, off, n):
    b = _bits(flat)
    sent = SENT32 if flat.dtype == torch.float32 else SENT16
    return bool((b[:PAD + off] == sent).all() and (b[PAD + off + n:] == sent).all())


def _values(rng, n):
    """n fp32 bit patterns drawn from the cast value set (ties, neighbours, subnormals ...), NaNs left out."""
    pats = R.cast_patterns()
    pats = pats[~np.isnan(pats.view(np.float32))]
    return pats[rng.integers(0, pats.size, n)]


def _permute(a, o, pc, ph):
    """f32-side [o][pc][ph] -> bf16-side [o][ph][pc] (flat)."""
    return a.reshape(o, pc, ph).transpose(0, 2, 1).reshape(-1) if pc else a


def _unpermute(a, o, pc, ph):
    return a.reshape(o, ph, pc).transpose(0, 2, 1).reshape(-1) if pc else a


def _run(cuda, dir_, specs, seed):
    """specs: (n, src_off, dst_off, (perm_c, perm_hw)) per tensor, one launch; checks values and guards."""
    from runtime import kernels as K

    rng = np.random.default_rng(seed)
    sdt, ddt = (torch.float32, torch.bfloat16) if dir_ == 0 else (torch.bfloat16, torch.float32)
    srcs, dsts, flats, wants = [], [], [], []
    for n, so, do, (pc, ph) in specs:
        f32_bits = _values(rng, n)
        rows = n // (pc * ph) if pc else 0
        if dir_ == 0:
            src_bits = f32_bits
            want = R.bf16_rne(_permute(f32_bits, rows, pc, ph).view(np.float32))
        else:
            src_bits = (f32_bits >> 16).astype(np.uint16)
            want = _unpermute(src_bits, rows, pc, ph).astype(np.uint32) << np.uint32(16)
        _, s = _buffer(cuda, sdt, n, so, src_bits)
        flat, d = _buffer(cuda, ddt, n, do)
        srcs.append(s)
        dsts.append(d)
        flats.append(flat)
        wants.append(want)
    K.cast_multi(dir_, srcs, dsts, [sp[3] for sp in specs])
    for i, (d, flat, want, (n, so, do, perm)) in enumerate(zip(dsts, flats, wants, specs)):
        got = _bits(d)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (i, n, so, do, perm, int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
        assert _guards_ok(flat, do, n), (i, n, so, do, perm, "guard overwritten")


def test_f32_to_bf16_rounds_to_nearest_even_on_every_pattern(cuda):
    from runtime import kernels as K

    pats = R.cast_patterns()
    want = R.bf16_rne(pats.view(np.float32))
    _, src = _buffer(cuda, torch.float32, pats.size, 0, pats)
    flat, dst = _buffer(cuda, torch.bfloat16, pats.size, 0)
    K.cast_multi(0, [src], [dst], [(0, 0)])
    got = _bits(dst)
    nan = np.isnan(pats.view(np.float32))
    assert nan.sum() > 500 and np.array_equal(R.is_nan_bf16(got), nan)  # NaN stays NaN, nothing else becomes one
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (bad.size, [(hex(int(pats[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
    assert _guards_ok(flat, 0, pats.size)
    big = np.flatnonzero(pats == 0x7F7FFFFF)[0]
    assert got[big] == 0x7F80  # the largest finite fp32 rounds to infinity


def test_bf16_to_f32_is_a_shift_on_every_pattern(cuda):
    from runtime import kernels as K

    pats = np.arange(65536, dtype=np.uint16)
    for off in (0, 1):  # the vector and the scalar branch
        _, src = _buffer(cuda, torch.bfloat16, pats.size, off, pats)
        flat, dst = _buffer(cuda, torch.float32, pats.size, 0)
        K.cast_multi(1, [src], [dst], [(0, 0)])
        assert np.array_equal(_bits(dst), pats.astype(np.uint32) << np.uint32(16))  # NaN payloads included
        assert _guards_ok(flat, 0, pats.size)


@pytest.mark.parametrize("dir_,src_off,dst_off", [(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 7), (0, 1, 1), (0, 1, 7),
                                                  (1, 0, 0), (1, 1, 0), (1, 7, 0), (1, 0, 1), (1, 1, 1), (1, 7, 1)])
def test_sizes_and_alignments(cuda, dir_, src_off, dst_off):
    _run(cuda, dir_, [(n, src_off, dst_off, (0, 0)) for n in SIZES], 100 * dir_ + 10 * src_off + dst_off)


# perm_c, perm_hw, rows, element offset of both sides
PERMS = [(128, 64, 3, 0), (64, 128, 3, 0), (12, 5, 3, 0), (1, 64, 3, 0), (64, 1, 3, 0), (5, 3, 4, 1)]


@pytest.mark.parametrize("dir_", [0, 1])
def test_permuted_rows(cuda, dir_):
    _run(cuda, dir_, [(o * pc * ph, off, off, (pc, ph)) for pc, ph, o, off in PERMS], 200 + dir_)


@pytest.mark.parametrize("dir_", [0, 1])
def test_table_of_48_tensors(cuda, dir_):
    offs = (0, 1, 7) if dir_ else (0, 1)
    specs = []
    for i in range(R.MAX_TENSORS):
        if i % 6 == 5:
            pc, ph, o, off = PERMS[(i // 6) % len(PERMS)]
            specs.append((o * pc * ph, off, off, (pc, ph)))
        else:
            specs.append((SIZES[i % len(SIZES)], offs[i % len(offs)], (i // 2) % 2, (0, 0)))
    assert len(specs) == 48 and specs[-1][3] != (0, 0)
    _run(cuda, dir_, specs, 300 + dir_)


def test_refusals(cuda, lib):
    from runtime import kernels as K

    def call(count, dir_, ns, pcs, phs):
        flats, srcs, dsts = [], [], []
        for n in ns:
            _, s = _buffer(cuda, torch.float32 if dir_ != 1 else torch.bfloat16, max(n, 1), 0, 0)
            flat, d = _buffer(cuda, torch.bfloat16 if dir_ != 1 else torch.float32, max(n, 1), 0)
            srcs.append(s)
            dsts.append(d)
            flats.append(flat)
        k = len(ns)
        rc = lib.bb_cast_multi(count, dir_, K._ptrs(srcs), K._ptrs(dsts), (C.c_int64 * k)(*ns), (C.c_int32 * k)(*pcs),
                               (C.c_int32 * k)(*phs), K._s(cuda))
        torch.cuda.synchronize()
        for flat in flats:  # a refused call launches nothing
            sent = SENT32 if flat.dtype == torch.float32 else SENT16
            assert bool((_bits(flat) == sent).all()) or rc == 0
        return rc

    assert call(1, 0, [8192], [128], [64]) == 0  # the largest permuted row
    assert call(1, 0, [8193], [8193], [1]) != 0  # perm_c * perm_hw = 8193
    assert call(1, 0, [8193 * 2], [3], [2731]) != 0
    assert call(1, 0, [100], [12], [5]) != 0  # n not a multiple of the row
    assert call(1, 0, [60], [-12], [5]) != 0  # perm_c < 0
    assert call(1, 0, [60], [12], [0]) != 0  # perm_hw = 0 with perm_c > 0
    assert call(1, 2, [64], [0], [0]) != 0  # dir = 2
    assert call(1, -1, [64], [0], [0]) != 0
    assert call(0, 0, [64], [0], [0]) != 0  # 0 tensors
    assert call(49, 0, [8] * 49, [0] * 49, [0] * 49) != 0  # 49 tensors
    assert call(2, 0, [64, 0], [0, 0], [0, 0]) != 0  # an empty tensor
    assert call(48, 1, [8] * 48, [0] * 48, [0] * 48) == 0
