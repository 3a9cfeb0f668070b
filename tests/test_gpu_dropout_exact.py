"""bb_dropout_forward (csrc/bb_optim.hip): the exact mask, not its statistics.

The kernel's draw is Philox4x32-10 with counter (element / 4, offset) and key seed, element e taking word e & 3 --
oracle/philox.py's layout -- so tests/_optim_ref.dropout_ref gives the kept set exactly: a kernel that used a Philox
lane twice or dropped a high word of the seed or the offset fails here.  Kept values are exactly bf16(y * scale)
(inf, -inf, NaN, -0.0 and negatives included), dropped ones +0, and after launch k the generator word reads
[seed, offset + k, 0, 0].  Sizes: one and two vectors, a partial block, exactly the 128-block cap, one vector past it,
and the unrolled grid-stride loop's tail.
"""
import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

HI = 1 << 32
SIZES = (8, 16, 2040, 262144, 262152, 4 * 262144 + 24)
WORDS = ((12345, 0), (3 * HI + 12345, 0), (12345, 9 * HI + 7), (HI - 1, HI - 1))
PROBS = (0.1, 0.5, 1e-10, 0.999)
SPECIALS = (0x7F80, 0xFF80, 0x7FC0, 0x8000, 0xC049)  # inf, -inf, NaN, -0.0, -3.14


def _launch(lib, y, p, rng):
    from runtime import kernels as K
    from runtime import lib as L

    L.check(lib.bb_dropout_forward(K._p(y), y.numel(), float(p), K._p(rng), K._s(y.device)), "bb_dropout_forward")


def _input(n, keep, seed):
    """bf16 patterns of n finite non-zero values of both signs, with SPECIALS at the first kept and the first
    dropped positions (as far as there are any)."""
    rng = np.random.default_rng(seed)
    y = R.bf16_rne((rng.standard_normal(n) * 4.0 + np.where(rng.random(n) < 0.5, -0.25, 0.25)).astype(np.float32))
    y[(y & 0x7FFF) == 0] = 0x3F80
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    for i, s in enumerate(SPECIALS):
        if i < kept.size:
            y[kept[i]] = s
        if i < dropped.size:
            y[dropped[i]] = s
    return y


def _expected(y_bits, keep, scale):
    wide = (y_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = R.bf16_rne(wide * scale)  # one fp32 product, rounded to bf16
    return np.where(keep, scaled, np.uint16(0))


@pytest.mark.parametrize("seed,offset", WORDS, ids=["low", "seed-high", "offset-high", "carry"])
@pytest.mark.parametrize("n", SIZES)
def test_mask_and_values_are_exact(cuda, lib, n, seed, offset):
    rng = torch.tensor([seed, offset, 0, 0], dtype=torch.int64, device=cuda)
    for k, p in enumerate(PROBS):
        keep, scale = R.dropout_ref(n, p, seed, offset + k)
        y0 = _input(n, keep, n + k)
        y = torch.from_numpy(y0.view(np.int16)).to(cuda).view(torch.bfloat16)
        _launch(lib, y, p, rng)
        got = y.view(torch.int16).cpu().numpy().view(np.uint16)
        want = _expected(y0, keep, scale)
        nan = R.is_nan_bf16(want)
        assert np.array_equal(R.is_nan_bf16(got), nan), (p, "NaN positions")
        bad = np.flatnonzero((got != want) & ~nan)
        assert bad.size == 0, (p, bad.size, int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])),
                               bool(keep[bad[0]]))
        assert rng.tolist() == [seed, offset + k + 1, 0, 0]
        if p == 1e-10:  # threshold 0, scale 1: everything kept, unchanged
            assert keep.all() and scale == np.float32(1.0) and np.array_equal(got[~nan], y0[~nan])
        if n >= 2040 and p in (0.1, 0.5):
            assert 0 < keep.sum() < n


def test_every_high_word_changes_the_mask(cuda, lib):
    n = 2040
    masks = []
    for seed, offset in WORDS:
        rng = torch.tensor([seed, offset, 0, 0], dtype=torch.int64, device=cuda)
        y = torch.ones(n, dtype=torch.bfloat16, device=cuda)
        _launch(lib, y, 0.5, rng)
        masks.append((y != 0).cpu().numpy())
        assert np.array_equal(masks[-1], R.dropout_ref(n, 0.5, seed, offset)[0])
    for m in masks[1:]:
        assert 0.3 < float((m != masks[0]).mean()) < 0.7
