"""bb_guided_loss_forward / _backward / _fused on the MI355X against the fp64 restatement (tests/_guided_ref.py).

Shapes: B = 1, 5, 67, 259 (259 rows span 65 blocks of 4 waves: the last-arriver hand-off and the row bound), mask
densities of 1, ~10% and 192 legal actions, the row kinds of ``_distill_ref.synthetic`` (empty M; M without S; exact
ties at the maximum of q; 0 beside -100000; a difference beyond -2^31), ratios at exactly 1, inside and outside the clip
range, zero advantages, and q from HIP bb_plan_values_pos on the positions of tests/_safe_positions.py; tau in
{0, 1, 50, 1e4}; the coefficient corners (1, c, e, 0), (0, c, 0, 1), (1, c, e, beta).

Tolerances, against fp64 (the project's, tests/test_gpu_ppo_kernels.py and tests/test_gpu_distill_loss.py): loss and
statistics rtol 1e-5 / atol 1e-6, clip_fraction within 2 / B, rows and agreement exact, dvalues rtol 1e-5 / atol 1e-9,
dlogits rtol 1e-4 / atol 1e-5 max|grad|.  Every case prints the kernel's and ``guided_loss_torch``'s (fp32, same
device) worst errors before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _distill_ref as D
import _guided_ref as R
import _safe_positions as S
from _guided_ref import BETA, CLIP, CORNERS, EC, VC, check_grads, check_stats

pytestmark = pytest.mark.gpu

TAUS = (0.0, 1.0, 50.0, 1e4)
SENTINEL = 12345.0
NAMES = ("logits", "values", "mask_bits", "actions", "old_logp", "adv", "ret", "q")


@functools.lru_cache(maxsize=None)
def _synthetic(B, density, kinds=True):
    return R.synthetic(B, seed=2000 + B, density=density, kinds=kinds)


@functools.lru_cache(maxsize=None)
def _searched(which):
    """Rows on set (a) or (b) of tests/_safe_positions.py: q from HIP bb_plan_values_pos (default weights, depth 2),
    the mask the sampling mask (the safe words, else the legal ones) of those positions."""
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K

    ref = S.reference_a() if which == "a" else S.reference_b()
    board, hand = S.tensors(ref["board"], ref["hand"], torch.device("cuda", 0))
    q = K.plan_values(board, hand, DEFAULT_WEIGHTS, 2, want=("q",))["q"].cpu().numpy()
    n = q.shape[0]
    assert ((q != D.INT64_MIN) == D.mask_bool(ref["legal"])).all()
    base = R.synthetic(n, seed=6, density="all", kinds=False)
    mb = ref["mode1"].view(np.int64).copy()
    M = D.mask_bool(mb)
    rng = np.random.default_rng(8)
    actions = np.array([rng.choice(np.flatnonzero(M[i])) if M[i].any() else 0 for i in range(n)], np.int64)
    ratio = np.tile([1.0, 1.1, 0.6, 1.4], n)[:n]
    old = (R.log_probs(base[0], mb, actions) - np.log(ratio)).astype(np.float32)
    return base[0], base[1], mb, actions, old, base[5], base[6], q


def _case(name):
    return _searched(name[-1]) if isinstance(name, str) else _synthetic(*name)


@functools.lru_cache(maxsize=None)
def _want(name, coefs, bf16=False, no_q=False):
    rows = list(_case(name))
    if bf16:
        rows[0] = torch.from_numpy(rows[0]).bfloat16().float().numpy()
        rows[1] = torch.from_numpy(rows[1]).bfloat16().float().numpy()
    if no_q:
        rows[7] = None
    return R.reference(*rows, CLIP, coefs, grad_loss=0.75)


def _dev(name, cuda, bf16=False):
    t = dict(zip(NAMES, (torch.from_numpy(a).to(cuda) for a in _case(name))))
    if bf16:
        t["logits"], t["values"] = t["logits"].bfloat16(), t["values"].bfloat16()
    return t


def _launch(form, t, coefs, g=None, cnt=None, coefs_dev=None, no_q=False):
    """One raw call of bb_guided_loss_<form> -> (stats, loss, dlogits, dvalues): one guard row around dlogits, a
    guard element around dvalues, guard words behind stats and loss, all checked."""
    from runtime import kernels as K
    from runtime import lib as L

    lib, dev, b = L.load(), t["logits"].device, t["logits"].shape[0]
    a = L.GuidedLossArgs(bf16=int(t["logits"].dtype == torch.bfloat16), B=b, clip=CLIP, policy_coef=coefs[0],
                         value_coef=coefs[1], entropy_coef=coefs[2], distill_coef=coefs[3], tau=coefs[4],
                         coefs_dev=None if coefs_dev is None else coefs_dev.data_ptr(),
                         **{k: t[k].data_ptr() for k in NAMES if not (no_q and k == "q")})
    keep = []
    stats = loss = dl = dv = None
    if form in ("forward", "fused"):
        ws = torch.empty((lib.bb_guided_loss_workspace_bytes(b) + 7) // 8, dtype=torch.float64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev) if cnt is None else cnt
        stats = torch.full((14,), SENTINEL, dtype=torch.float32, device=dev)
        loss = torch.full((2,), SENTINEL, dtype=torch.float32, device=dev)
        a.ws, a.cnt, a.stats, a.loss = ws.data_ptr(), cnt.data_ptr(), stats.data_ptr(), loss.data_ptr()
        keep += [ws, cnt]
    if form in ("backward", "fused"):
        dl = torch.full((b + 2, 192), SENTINEL, dtype=t["logits"].dtype, device=dev)
        dv = torch.full((b + 2,), SENTINEL, dtype=t["values"].dtype, device=dev)
        a.grad_loss, a.dlogits, a.dvalues = g.data_ptr(), dl[1].data_ptr(), dv[1:].data_ptr()
    L.check(getattr(lib, f"bb_guided_loss_{form}")(C.byref(a), K._s(dev)), f"bb_guided_loss_{form}")
    torch.cuda.synchronize(dev)
    if stats is not None:
        assert stats[12:].tolist() == [SENTINEL] * 2 and loss[1].item() == SENTINEL, "written past stats / loss"
        assert cnt.item() == 0, "the counter was not re-armed"
    if dl is not None:
        assert (dl[0] == SENTINEL).all() and (dl[-1] == SENTINEL).all(), "written outside dlogits [B][192]"
        assert bool(dv[0] == SENTINEL) and bool(dv[-1] == SENTINEL), "written outside dvalues [B]"
    return (stats[:12] if stats is not None else None, loss[0] if loss is not None else None,
            dl[1:-1] if dl is not None else None, dv[1:-1] if dv is not None else None)


def _np(t):
    return t.double().cpu().numpy()


def _errors(label, stats, dl, dv, want):
    es = np.abs(_np(stats) - want["stats"])
    print(f"  {label}: |err| " + " ".join(f"{k} {e:.2e}" for k, e in zip(R.STATS, es))
          + f" dlogits {np.abs(_np(dl) - want['dlogits']).max():.2e} (max|grad| {np.abs(want['dlogits']).max():.2e})"
          + f" dvalues {np.abs(_np(dv) - want['dvalues']).max():.2e}")


def _torch_fp32(t, coefs, g):
    from agents.ppo import guided_loss_torch

    x, v = t["logits"].float().clone().requires_grad_(True), t["values"].float().clone().requires_grad_(True)
    loss, stats = guided_loss_torch(x, v, *(t[k] for k in NAMES[2:]), CLIP, coefs)
    loss.backward(g[0])
    return stats, x.grad, v.grad


CASES = ([((B, "mixed"), tau, "guided") for B in (1, 5, 67, 259) for tau in TAUS]
         + [((67, d), tau, c) for d in ("one", "tenth", "all") for tau in (0.0, 50.0) for c in CORNERS]
         + [((259, "mixed"), 50.0, c) for c in ("ppo", "distill+critic")]
         + [(f"searched-{w}", tau, "guided") for w in "ab" for tau in TAUS])


@pytest.mark.parametrize("name,tau,corner", CASES, ids=[f"{n}-tau{t:g}-{c}" for n, t, c in CASES])
def test_fused_matches_fp64(cuda, name, tau, corner):
    coefs = (*CORNERS[corner], tau)
    t = _dev(name, cuda)
    want = _want(name, coefs)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    stats, loss, dl, dv = _launch("fused", t, coefs, g)
    B = t["logits"].shape[0]
    print(f"\n{name} tau {tau:g} {corner}: B {B}, rows {int(want['stats'][11])}, total {want['stats'][3]:.6f}")
    _errors("kernel", stats, dl, dv, want)
    _errors("torch fp32", *_torch_fp32(t, coefs, g), want)
    assert loss.item() == stats[3].item()
    check_stats(_np(stats), want["stats"], B)
    check_grads(_np(dl), _np(dv), want, t["mask_bits"].cpu().numpy())


@pytest.mark.parametrize("corner", list(CORNERS))
def test_forward_and_backward_match_fp64(cuda, corner):
    name, coefs = (259, "mixed"), (*CORNERS[corner], 50.0)
    t = _dev(name, cuda)
    want = _want(name, coefs)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    stats, loss, _, _ = _launch("forward", t, coefs)
    _, _, dl, dv = _launch("backward", t, coefs, g)
    assert loss.item() == stats[3].item()
    check_stats(_np(stats), want["stats"], 259)
    check_grads(_np(dl), _np(dv), want, t["mask_bits"].cpu().numpy())


def _same(a, b):
    w = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(w), b.view(w))


@pytest.mark.parametrize("name,tau", [((259, "mixed"), 50.0), ((5, "mixed"), 0.0), ("searched-b", 1.0)],
                         ids=["259", "5", "searched"])
def test_fused_is_forward_plus_backward_and_repeats(cuda, name, tau):
    t = _dev(name, cuda)
    coefs = (*CORNERS["guided"], tau)
    g = torch.tensor([-1.25], dtype=torch.float32, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)  # one counter through all launches: each re-arms it
    fs, fl, fd, fv = _launch("fused", t, coefs, g, cnt)
    s1, l1, _, _ = _launch("forward", t, coefs, cnt=cnt)
    _, _, d1, v1 = _launch("backward", t, coefs, g)
    fs2, fl2, fd2, fv2 = _launch("fused", t, coefs, g, cnt)
    for a, b in ((fs, s1), (fl, l1), (fd, d1), (fv, v1), (fs, fs2), (fl, fl2), (fd, fd2), (fv, fv2)):
        assert _same(a, b)


@pytest.mark.parametrize("tau", [0.0, 50.0])
def test_bf16_logits_and_values(cuda, tau):
    """bf16 inputs are the f32 path on the widened values; the gradients are its bf16 rounding (to nearest even)."""
    name, coefs = (259, "mixed"), (*CORNERS["guided"], tau)
    tb = _dev(name, cuda, bf16=True)
    tw = dict(tb, logits=tb["logits"].float(), values=tb["values"].float())
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    bs, bl, bd, bv = _launch("fused", tb, coefs, g)
    ws, wl, wd, wv = _launch("fused", tw, coefs, g)
    assert bd.dtype == torch.bfloat16 and bv.dtype == torch.bfloat16
    assert _same(bs, ws) and torch.equal(bl, wl)
    assert _same(bd, wd.bfloat16()) and _same(bv, wv.bfloat16())
    check_stats(_np(bs), _want(name, coefs, bf16=True)["stats"], 259)
    _, _, d2, v2 = _launch("backward", tb, coefs, g)
    assert _same(bd, d2) and _same(bv, v2)


def test_coefs_dev_equals_the_scalars(cuda):
    t = _dev((259, "mixed"), cuda)
    coefs = (0.7, 0.4, 0.03, 0.6, 20.0)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    cdev = torch.tensor(coefs, dtype=torch.float32, device=cuda)
    want = _launch("fused", t, coefs, g)
    got = _launch("fused", t, (9.0, 9.0, 9.0, 9.0, 9.0), g, coefs_dev=cdev)  # the scalars are overridden
    assert all(_same(a, b) for a, b in zip(got, want))
    fs, fl, _, _ = _launch("forward", t, (0.0,) * 5, coefs_dev=cdev)
    _, _, bd, bv = _launch("backward", t, (0.0,) * 5, g, coefs_dev=cdev)
    assert all(_same(a, b) for a, b in zip((fs, fl, bd, bv), want))


def test_without_q_is_the_ppo_kernel(cuda):
    """q == NULL, distill_coef = 0 against bb_ppo_loss_fused on the expanded f32 mask (no empty-M row: the PPO kernel
    has no rule for one)."""
    from runtime import kernels as K
    from runtime import lib as L

    name, coefs = (259, "mixed", False), (1.0, VC, EC, 0.0, 50.0)
    t = _dev(name, cuda)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    stats, loss, dl, dv = _launch("fused", t, coefs, g, no_q=True)
    assert not stats[6:].any()
    want = _want(name, coefs, no_q=True)
    check_stats(_np(stats), want["stats"], 259)
    check_grads(_np(dl), _np(dv), want, t["mask_bits"].cpu().numpy())
    lib, b = L.load(), 259
    mask = K.mask_bits_to_bool(t["mask_bits"]).float().contiguous()
    ws = torch.empty((lib.bb_ppo_loss_workspace_bytes(b) + 7) // 8, dtype=torch.float64, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    ps, pl = torch.empty(6, dtype=torch.float32, device=cuda), torch.empty(1, dtype=torch.float32, device=cuda)
    pd, pv = torch.empty_like(t["logits"]), torch.empty_like(t["values"])
    a = L.PpoLossArgs(logits=t["logits"].data_ptr(), values=t["values"].data_ptr(), bf16=0, mask=mask.data_ptr(),
                      actions=t["actions"].data_ptr(), old_logp=t["old_logp"].data_ptr(), adv=t["adv"].data_ptr(),
                      ret=t["ret"].data_ptr(), B=b, clip=CLIP, value_coef=VC, entropy_coef=EC, grad_loss=g.data_ptr(),
                      dlogits=pd.data_ptr(), dvalues=pv.data_ptr(), ws=ws.data_ptr(), cnt=cnt.data_ptr(),
                      stats=ps.data_ptr(), loss=pl.data_ptr())
    L.check(lib.bb_ppo_loss_fused(C.byref(a), K._s(cuda)), "bb_ppo_loss_fused")
    torch.cuda.synchronize(cuda)
    # the same row function (csrc/bb_loss_rows.h ppo_row) and the same hand-off: equal, +-0 in dlogits aside
    assert torch.equal(stats[:6], ps) and loss.item() == pl.item()
    assert torch.equal(dv, pv)
    assert torch.equal(dl, pd)


@pytest.mark.parametrize("tau", [0.0, 50.0])
def test_ppo_coefficients_zero_is_the_distill_kernel(cuda, tau):
    from runtime import kernels as K
    from runtime import lib as L

    t = _dev((259, "mixed"), cuda)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    stats, loss, dl, dv = _launch("fused", t, (0.0, 0.0, 0.0, 1.0, tau), g)
    lib, b = L.load(), 259
    ws = torch.empty((lib.bb_distill_loss_workspace_bytes(b) + 7) // 8, dtype=torch.float64, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    ds, dloss = torch.empty(6, dtype=torch.float32, device=cuda), torch.empty(1, dtype=torch.float32, device=cuda)
    dd = torch.empty_like(t["logits"])
    a = L.DistillLossArgs(logits=t["logits"].data_ptr(), bf16=0, mask_bits=t["mask_bits"].data_ptr(),
                          q=t["q"].data_ptr(), B=b, tau=tau, grad_loss=g.data_ptr(), dlogits=dd.data_ptr(),
                          ws=ws.data_ptr(), cnt=cnt.data_ptr(), stats=ds.data_ptr(), loss=dloss.data_ptr())
    L.check(lib.bb_distill_loss_fused(C.byref(a), K._s(cuda)), "bb_distill_loss_fused")
    torch.cuda.synchronize(cuda)
    # the same row function (csrc/bb_loss_rows.h distill_row) and the same hand-off: equal, +-0 in dlogits aside
    assert torch.equal(stats[6:], ds)
    assert stats[3].item() == ds[0].item()  # total = 1 * cross-entropy
    assert loss.item() == stats[3].item() and not dv.any()
    assert torch.equal(dl, dd)


def test_graph_captured_on_the_first_launch(cuda):
    """Captured before any eager launch (a fresh counter, nothing warmed), replayed on changed inputs and a changed
    coefs_dev; each replay equals an eager call with those scalars."""
    from runtime import kernels as K
    from runtime import lib as L

    lib = L.load()
    t = {k: v.clone() for k, v in _dev((259, "mixed"), cuda).items()}
    b = 259
    g = torch.tensor([1.0], dtype=torch.float32, device=cuda)
    cdev = torch.tensor([1.0, VC, EC, BETA, 50.0], dtype=torch.float32, device=cuda)
    ws = torch.empty((lib.bb_guided_loss_workspace_bytes(b) + 7) // 8, dtype=torch.float64, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    stats = torch.zeros(12, dtype=torch.float32, device=cuda)
    loss = torch.zeros(1, dtype=torch.float32, device=cuda)
    dl, dv = torch.zeros_like(t["logits"]), torch.zeros_like(t["values"])
    a = L.GuidedLossArgs(bf16=0, B=b, clip=CLIP, policy_coef=0.0, value_coef=0.0, entropy_coef=0.0, distill_coef=0.0,
                         tau=0.0, coefs_dev=cdev.data_ptr(), grad_loss=g.data_ptr(), dlogits=dl.data_ptr(),
                         dvalues=dv.data_ptr(), ws=ws.data_ptr(), cnt=cnt.data_ptr(), stats=stats.data_ptr(),
                         loss=loss.data_ptr(), **{k: t[k].data_ptr() for k in NAMES})
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(lib.bb_guided_loss_fused(C.byref(a), K._s(cuda)), "bb_guided_loss_fused")
    for seed, coefs in ((1, (1.0, VC, EC, 0.5, 50.0)), (2, (0.0, 0.25, 0.0, 1.0, 0.0))):
        for k, arr in zip(NAMES, R.synthetic(b, seed=seed, density="tenth")):
            t[k].copy_(torch.from_numpy(arr))
        g.fill_(0.5 * seed)
        cdev.copy_(torch.tensor(coefs, dtype=torch.float32))
        graph.replay()
        torch.cuda.synchronize(cuda)
        es, el, ed, ev = _launch("fused", t, coefs, g)
        assert _same(stats, es) and loss[0].item() == el.item() and _same(dl, ed) and _same(dv, ev)
        assert cnt.item() == 0


def test_autograd_function_and_wrapper(cuda):
    """runtime.kernels.guided_loss / GuidedLossFunction: the seeded path hands the fused launch's gradients over, any
    other gradient runs the backward kernel; both are the raw calls bit for bit, with scalars or coefs_dev."""
    from runtime import kernels as K

    t = _dev((67, "mixed"), cuda)
    coefs = (*CORNERS["guided"], 50.0)
    one = torch.ones((), dtype=torch.float32, device=cuda)
    rs, rl, rd, rv = _launch("fused", t, coefs, one.reshape(1))
    rows = [t[k] for k in NAMES]
    l0, s0 = K.guided_loss(*rows, CLIP, coefs)
    assert torch.equal(s0, rs) and l0.item() == rl.item()
    cdev = torch.tensor(coefs, dtype=torch.float32, device=cuda)
    for seed, dev in ((one, None), (None, None), (one, cdev), (None, cdev)):
        x, v = t["logits"].clone().requires_grad_(True), t["values"].clone().requires_grad_(True)
        loss, stats = K.GuidedLossFunction.apply(x, v, *rows[2:], CLIP, coefs if dev is None else (0.0,) * 5, dev,
                                                 seed)
        assert not stats.requires_grad
        loss.backward(one) if seed is not None else loss.backward()
        assert torch.equal(stats, rs) and _same(x.grad, rd) and _same(v.grad, rv)
