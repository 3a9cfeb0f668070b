"""bb_distill_loss_forward / _backward / _fused on the MI355X against the fp64 restatement (tests/_distill_ref.py).

Shapes: B = 1, 5, 67, 259 (259 rows span 65 blocks of 4 waves: the last-arriver hand-off and the row bound), mask
densities of 1, ~10% and 192 legal actions, the row kinds of ``_distill_ref.synthetic`` (empty M; M without S; exact
ties at the maximum of q; 0 beside -100000; a difference beyond -2^31), and q from HIP bb_plan_values_pos on the
positions of tests/_safe_positions.py; tau in {0, 1, 50, 1e4}.

Tolerances, against fp64: loss and statistics rtol 1e-5 / atol 1e-6, dlogits rtol 1e-4 / atol 1e-5 max|grad| (those
of test_fused_ppo_loss_matches_torch); agreement and rows exact.  Every case prints the kernel's and
``distill_loss_torch``'s (fp32, same device) worst errors before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _distill_ref as R
import _safe_positions as S

pytestmark = pytest.mark.gpu

TAUS = (0.0, 1.0, 50.0, 1e4)
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _synthetic(B, density):
    return R.synthetic(B, seed=1000 + B, density=density)


@functools.lru_cache(maxsize=None)
def _searched(which):
    """(logits, mask words, q) with q from HIP bb_plan_values_pos (default weights, depth 2) on set (a) or (b) of
    tests/_safe_positions.py, under the sampling mask (the safe words, else the legal ones) of those positions."""
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K

    ref = S.reference_a() if which == "a" else S.reference_b()
    board, hand = S.tensors(ref["board"], ref["hand"], torch.device("cuda", 0))
    q = K.plan_values(board, hand, DEFAULT_WEIGHTS, 2, want=("q",))["q"].cpu().numpy()
    n = q.shape[0]
    assert ((q != R.INT64_MIN) == R.mask_bool(ref["legal"])).all()
    print(f"searched set ({which}): {n} positions, {int(((q != R.INT64_MIN) & (q < -50000)).sum())} dead afterstates")
    logits = (np.random.default_rng(5).standard_normal((n, 192)) * 2.0).astype(np.float32)
    return logits, ref["mode1"].view(np.int64).copy(), q


def _case(name):
    return _searched(name[-1]) if isinstance(name, str) and name.startswith("searched") else _synthetic(*name)


@functools.lru_cache(maxsize=None)
def _want(name, tau, bf16=False):
    logits, mb, q = _case(name)
    if bf16:
        logits = torch.from_numpy(logits).bfloat16().float().numpy()
    return R.reference(logits, mb, q, tau, grad_loss=0.75)


def _dev(name, cuda, bf16=False):
    logits, mb, q = _case(name)
    x = torch.from_numpy(logits).to(cuda)
    return (x.bfloat16() if bf16 else x), torch.from_numpy(mb).to(cuda), torch.from_numpy(q).to(cuda)


def _launch(form, x, mb, q, tau, g=None, cnt=None, guard=True):
    """One raw call of bb_distill_loss_<form> -> (stats, loss, dlogits with one guard row before and after)."""
    from runtime import kernels as K
    from runtime import lib as L

    lib, dev, b = L.load(), x.device, x.shape[0]
    a = L.DistillLossArgs(logits=x.data_ptr(), bf16=int(x.dtype == torch.bfloat16), mask_bits=mb.data_ptr(),
                          q=q.data_ptr(), B=b, tau=tau)
    keep = []
    stats = loss = dl = None
    if form in ("forward", "fused"):
        ws = torch.empty((lib.bb_distill_loss_workspace_bytes(b) + 7) // 8, dtype=torch.float64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev) if cnt is None else cnt
        stats = torch.full((8,), SENTINEL, dtype=torch.float32, device=dev)
        loss = torch.full((2,), SENTINEL, dtype=torch.float32, device=dev)
        a.ws, a.cnt, a.stats, a.loss = ws.data_ptr(), cnt.data_ptr(), stats.data_ptr(), loss.data_ptr()
        keep += [ws, cnt]
    if form in ("backward", "fused"):
        dl = torch.full((b + 2, 192), SENTINEL, dtype=x.dtype, device=dev)
        a.grad_loss, a.dlogits = g.data_ptr(), dl[1].data_ptr()
    L.check(getattr(lib, f"bb_distill_loss_{form}")(C.byref(a), K._s(dev)), f"bb_distill_loss_{form}")
    torch.cuda.synchronize(dev)
    if stats is not None:
        assert stats[6:].tolist() == [SENTINEL] * 2 and loss[1].item() == SENTINEL, "written past stats / loss"
        if cnt is not None:
            assert cnt.item() == 0, "the counter was not re-armed"
    if dl is not None:
        assert (dl[0] == SENTINEL).all() and (dl[-1] == SENTINEL).all(), "written outside [B][192]"
    return (stats[:6] if stats is not None else None, loss[0] if loss is not None else None,
            dl[1:-1] if dl is not None else None)


def _errors(label, got_stats, got_dl, want):
    es = np.abs(got_stats.double().cpu().numpy()[:4] - want["stats"][:4])
    ed = np.abs(got_dl.double().cpu().numpy() - want["dlogits"]).max()
    print(f"  {label}: |err| ce {es[0]:.2e} kl {es[1]:.2e} ht {es[2]:.2e} hp {es[3]:.2e} dlogits {ed:.2e} "
          f"(max|grad| {np.abs(want['dlogits']).max():.2e})")


CASES = ([((B, "mixed"), tau) for B in (1, 5, 67, 259) for tau in TAUS]
         + [((67, d), tau) for d in ("one", "tenth", "all") for tau in (0.0, 50.0)]
         + [(f"searched-{w}", tau) for w in "ab" for tau in TAUS])


@pytest.mark.parametrize("name,tau", CASES, ids=[f"{n}-tau{t:g}" for n, t in CASES])
def test_fused_matches_fp64(cuda, name, tau):
    from agents.ppo import distill_loss_torch

    x, mb, q = _dev(name, cuda)
    want = _want(name, tau)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    stats, loss, dl = _launch("fused", x, mb, q, tau, g)
    xt = x.clone().requires_grad_(True)
    tl, ts = distill_loss_torch(xt, mb, q, tau)
    tl.backward(g[0])
    print(f"\n{name} tau {tau:g}: B {x.shape[0]}, rows {int(want['stats'][5])}, ce {want['stats'][0]:.6f}")
    _errors("kernel", stats, dl, want)
    _errors("torch fp32", ts, xt.grad, want)
    got = stats.double().cpu().numpy()
    np.testing.assert_allclose(got[:4], want["stats"][:4], rtol=1e-5, atol=1e-6)
    assert loss.item() == stats[0].item()
    B = x.shape[0]
    assert got[4] == np.float32(want["stats"][4]) and round(got[4] * B) == round(want["stats"][4] * B)  # exact
    assert got[5] == want["stats"][5]
    d = dl.double().cpu().numpy()
    np.testing.assert_allclose(d, want["dlogits"], rtol=1e-4, atol=1e-5 * np.abs(want["dlogits"]).max())
    M = R.mask_bool(mb.cpu().numpy())
    assert not d[~M].any(), "gradient outside the mask"
    assert not d[~want["has"]].any(), "gradient in a row with empty S"
    if tau == 0:  # exactly one target entry per row, the lowest argmax of q: the one entry with pi - 1 <= 0 ...
        rows = np.flatnonzero(want["has"])
        neg = d[rows] < 0
        many = M[rows].sum(axis=1) > 1
        assert (neg.sum(axis=1)[many] == 1).all()
        assert np.array_equal(np.argmax(neg, axis=1)[many], want["qarg"][rows][many])
        assert not d[rows][~many].any()  # ... and with one legal action pi = t = 1: no gradient at all


@pytest.mark.parametrize("name,tau", [((259, "mixed"), 50.0), ((5, "mixed"), 0.0), ("searched-b", 1.0)],
                         ids=["259", "5", "searched"])
def test_fused_is_forward_plus_backward_and_repeats(cuda, name, tau):
    x, mb, q = _dev(name, cuda)
    g = torch.tensor([-1.25], dtype=torch.float32, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)  # one counter through all launches: each re-arms it
    fs, fl, fd = _launch("fused", x, mb, q, tau, g, cnt)
    s1, l1, _ = _launch("forward", x, mb, q, tau, cnt=cnt)
    _, _, d1 = _launch("backward", x, mb, q, tau, g)
    fs2, fl2, fd2 = _launch("fused", x, mb, q, tau, g, cnt)
    for a, b in ((fs, s1), (fl, l1), (fd, d1), (fs, fs2), (fl, fl2), (fd, fd2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("tau", [0.0, 50.0])
def test_bf16_logits(cuda, tau):
    """bf16 logits are the f32 path on the widened values; dlogits is its bf16 rounding (to nearest even)."""
    name = (259, "mixed")
    xb, mb, q = _dev(name, cuda, bf16=True)
    g = torch.tensor([0.75], dtype=torch.float32, device=cuda)
    bs, bl, bd = _launch("fused", xb, mb, q, tau, g)
    ws, wl, wd = _launch("fused", xb.float(), mb, q, tau, g)
    assert bd.dtype == torch.bfloat16
    assert torch.equal(bs.view(torch.int32), ws.view(torch.int32)) and torch.equal(bl, wl)
    assert torch.equal(bd.view(torch.int16), wd.bfloat16().view(torch.int16))
    want = _want(name, tau, bf16=True)
    np.testing.assert_allclose(bs.double().cpu().numpy()[:4], want["stats"][:4], rtol=1e-5, atol=1e-6)
    _, _, d2 = _launch("backward", xb, mb, q, tau, g)
    assert torch.equal(bd.view(torch.int16), d2.view(torch.int16))


def test_graph_captured_on_the_first_launch(cuda):
    """Captured before any eager launch (a fresh counter, nothing warmed), replayed on changed inputs."""
    from runtime import kernels as K
    from runtime import lib as L

    lib = L.load()
    x, mb, q = (t.clone() for t in _dev((259, "mixed"), cuda))
    b = x.shape[0]
    g = torch.tensor([1.0], dtype=torch.float32, device=cuda)
    ws = torch.empty((lib.bb_distill_loss_workspace_bytes(b) + 7) // 8, dtype=torch.float64, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    stats = torch.zeros(6, dtype=torch.float32, device=cuda)
    loss = torch.zeros(1, dtype=torch.float32, device=cuda)
    dl = torch.zeros_like(x)
    a = L.DistillLossArgs(logits=x.data_ptr(), bf16=0, mask_bits=mb.data_ptr(), q=q.data_ptr(), B=b, tau=50.0,
                          grad_loss=g.data_ptr(), dlogits=dl.data_ptr(), ws=ws.data_ptr(), cnt=cnt.data_ptr(),
                          stats=stats.data_ptr(), loss=loss.data_ptr())
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(lib.bb_distill_loss_fused(C.byref(a), K._s(cuda)), "bb_distill_loss_fused")
    for seed in (1, 2):
        nx, nmb, nq = R.synthetic(b, seed=seed, density="tenth")
        x.copy_(torch.from_numpy(nx))
        mb.copy_(torch.from_numpy(nmb))
        q.copy_(torch.from_numpy(nq))
        g.fill_(0.5 * seed)
        graph.replay()
        torch.cuda.synchronize(cuda)
        es, el, ed = _launch("fused", x, mb, q, 50.0, g)
        assert torch.equal(stats.view(torch.int32), es.view(torch.int32)) and loss[0].item() == el.item()
        assert torch.equal(dl.view(torch.int32), ed.view(torch.int32))
        assert cnt.item() == 0


def test_autograd_function_and_wrapper(cuda):
    """runtime.kernels.distill_loss / DistillLossFunction: the seeded path hands the fused launch's gradient over,
    any other gradient runs the backward kernel; both are the raw calls bit for bit."""
    from runtime import kernels as K

    x, mb, q = _dev((67, "mixed"), cuda)
    one = torch.ones((), dtype=torch.float32, device=cuda)
    rs, rl, rd = _launch("fused", x, mb, q, 50.0, one.reshape(1))
    l0, s0 = K.distill_loss(x, mb, q, 50.0)
    assert torch.equal(s0, rs) and l0.item() == rl.item()
    for seed in (one, None):
        xt = x.clone().requires_grad_(True)
        loss, stats = K.DistillLossFunction.apply(xt, mb, q, 50.0, seed)
        assert not stats.requires_grad
        loss.backward(one) if seed is not None else loss.backward()
        assert torch.equal(stats, rs) and torch.equal(xt.grad.view(torch.int32), rd.view(torch.int32))
