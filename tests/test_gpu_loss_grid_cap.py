"""The three fused loss kernels past their grid cap of 4,096 blocks: B = 4 * 4096 + 5 = 16,389 rows, so every wave
takes a second row (and five waves a fifth) through the row-stride loop, which no other test reaches.

Fused, f32, against the fp64 restatements (tests/_guided_ref.py, tests/_distill_ref.py) at the tolerances of
tests/test_gpu_guided_loss.py and tests/test_gpu_distill_loss.py, and fused == forward + backward bit for bit.

The restatements walk the rows in Python (5 s for 16,389 guided rows), so the batch is 27 copies of 607 seeded rows
(16,389 = 27 * 607; row i is row i % 607, and the stride of 16,384 rows is no multiple of 607).  The losses are means
over rows, so the restatement of the 607 rows gives the batch's: the same means, 27 times the row count, and its
gradients divided by 27.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _distill_ref as D
import _guided_ref as R
import test_gpu_distill_loss as TD
import test_gpu_guided_loss as TG
from _guided_ref import CLIP, CORNERS, EC, VC

pytestmark = pytest.mark.gpu

BASE, COPIES = 607, 27
B = BASE * COPIES
TAU, G = 50.0, 0.75
assert B == 4 * 4096 + 5


@functools.lru_cache(maxsize=None)
def _base():
    """607 rows without the special kinds: the PPO kernel has no rule for a row with empty M."""
    return R.synthetic(BASE, seed=2000 + B, density="mixed", kinds=False)


def _copies(a):
    return np.tile(a, (COPIES,) + (1,) * (a.ndim - 1))


def _dev(cuda):
    return {k: torch.from_numpy(_copies(a)).to(cuda) for k, a in zip(TG.NAMES, _base())}


def _tiled(want, keys):
    """The restatement of the 607 rows -> that of the 27 copies."""
    out = dict(want)
    for k in keys:
        out[k] = _copies(want[k])
    for k in ("dlogits", "dvalues"):
        if k in out:
            out[k] = out[k] / COPIES
    out["stats"] = want["stats"].copy()
    out["stats"][-1] *= COPIES  # rows
    return out


def _np(t):
    return t.double().cpu().numpy()


def _same(pairs):
    for a, b in pairs:
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_guided(cuda):
    coefs = (*CORNERS["guided"], TAU)
    t = _dev(cuda)
    want = _tiled(R.reference(*_base(), CLIP, coefs, grad_loss=G), ("dlogits", "dvalues", "live"))
    g = torch.tensor([G], dtype=torch.float32, device=cuda)
    stats, loss, dl, dv = TG._launch("fused", t, coefs, g)
    TG._errors("kernel", stats, dl, dv, want)
    assert loss.item() == stats[3].item()
    R.check_stats(_np(stats), want["stats"], B)
    R.check_grads(_np(dl), _np(dv), want, t["mask_bits"].cpu().numpy())
    s1, l1, _, _ = TG._launch("forward", t, coefs)
    _, _, d1, v1 = TG._launch("backward", t, coefs, g)
    _same(((stats, s1), (loss, l1), (dl, d1), (dv, v1)))


def test_distill(cuda):
    t = _dev(cuda)
    logits, _, mb, _, _, _, _, q = _base()
    want = _tiled(D.reference(logits, mb, q, TAU, grad_loss=G), ("dlogits", "has"))
    g = torch.tensor([G], dtype=torch.float32, device=cuda)
    x, mbd, qd = t["logits"], t["mask_bits"], t["q"]
    stats, loss, dl = TD._launch("fused", x, mbd, qd, TAU, g)
    TD._errors("kernel", stats, dl, want)
    got = _np(stats)
    np.testing.assert_allclose(got[:4], want["stats"][:4], rtol=1e-5, atol=1e-6)
    assert loss.item() == stats[0].item()
    assert got[4] == np.float32(want["stats"][4]) and round(got[4] * B) == round(want["stats"][4] * B)  # exact
    assert got[5] == want["stats"][5]
    d = _np(dl)
    np.testing.assert_allclose(d, want["dlogits"], rtol=1e-4, atol=1e-5 * np.abs(want["dlogits"]).max())
    assert not d[~D.mask_bool(mbd.cpu().numpy())].any(), "gradient outside the mask"
    assert not d[~want["has"]].any(), "gradient in a row with empty S"
    s1, l1, _ = TD._launch("forward", x, mbd, qd, TAU)
    _, _, d1 = TD._launch("backward", x, mbd, qd, TAU, g)
    _same(((stats, s1), (loss, l1), (dl, d1)))


def _ppo_launch(form, t, mask, g):
    """One raw call of bb_ppo_loss_<form> -> (stats, loss, dlogits, dvalues), guard rows around the gradients."""
    from runtime import kernels as K
    from runtime import lib as L

    lib, dev = L.load(), mask.device
    a = L.PpoLossArgs(logits=t["logits"].data_ptr(), values=t["values"].data_ptr(), bf16=0, mask=mask.data_ptr(),
                      actions=t["actions"].data_ptr(), old_logp=t["old_logp"].data_ptr(), adv=t["adv"].data_ptr(),
                      ret=t["ret"].data_ptr(), B=B, clip=CLIP, value_coef=VC, entropy_coef=EC)
    stats = loss = dl = dv = None
    if form in ("forward", "fused"):
        ws = torch.empty((lib.bb_ppo_loss_workspace_bytes(B) + 7) // 8, dtype=torch.float64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        stats = torch.full((8,), TG.SENTINEL, dtype=torch.float32, device=dev)
        loss = torch.full((2,), TG.SENTINEL, dtype=torch.float32, device=dev)
        a.ws, a.cnt, a.stats, a.loss = ws.data_ptr(), cnt.data_ptr(), stats.data_ptr(), loss.data_ptr()
    if form in ("backward", "fused"):
        dl = torch.full((B + 2, 192), TG.SENTINEL, dtype=torch.float32, device=dev)
        dv = torch.full((B + 2,), TG.SENTINEL, dtype=torch.float32, device=dev)
        a.grad_loss, a.dlogits, a.dvalues = g.data_ptr(), dl[1].data_ptr(), dv[1:].data_ptr()
    L.check(getattr(lib, f"bb_ppo_loss_{form}")(C.byref(a), K._s(dev)), f"bb_ppo_loss_{form}")
    torch.cuda.synchronize(dev)
    if stats is not None:
        assert stats[6:].tolist() == [TG.SENTINEL] * 2 and loss[1].item() == TG.SENTINEL, "written past stats / loss"
        assert cnt.item() == 0, "the counter was not re-armed"
    if dl is not None:
        assert (dl[0] == TG.SENTINEL).all() and (dl[-1] == TG.SENTINEL).all(), "written outside dlogits [B][192]"
        assert bool(dv[0] == TG.SENTINEL) and bool(dv[-1] == TG.SENTINEL), "written outside dvalues [B]"
    return (stats[:6] if stats is not None else None, loss[0] if loss is not None else None,
            dl[1:-1] if dl is not None else None, dv[1:-1] if dv is not None else None)


def test_ppo(cuda):
    """bb_ppo_loss_* on the expanded f32 mask against the restatement's PPO half (q = None, distill_coef = 0)."""
    from runtime import kernels as K

    t = _dev(cuda)
    want = _tiled(R.reference(*_base()[:7], None, CLIP, (1.0, VC, EC, 0.0, TAU), grad_loss=G),
                  ("dlogits", "dvalues", "live"))
    mask = K.mask_bits_to_bool(t["mask_bits"]).float().contiguous()
    g = torch.tensor([G], dtype=torch.float32, device=cuda)
    stats, loss, dl, dv = _ppo_launch("fused", t, mask, g)
    got = np.concatenate([_np(stats), np.zeros(6)])
    print("  kernel: |err| " + " ".join(f"{k} {e:.2e}" for k, e in zip(R.STATS[:6], np.abs(got - want["stats"]))))
    assert loss.item() == stats[3].item()
    R.check_stats(got, want["stats"], B)
    R.check_grads(_np(dl), _np(dv), want, t["mask_bits"].cpu().numpy())
    s1, l1, _, _ = _ppo_launch("forward", t, mask, None)
    _, _, d1, v1 = _ppo_launch("backward", t, mask, g)
    _same(((stats, s1), (loss, l1), (dl, d1), (dv, v1)))
