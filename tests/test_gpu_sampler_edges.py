"""bb_masked_sample / bb_masked_sample_dstep on the MI355X, through the C ABI, on the corner rows of
tests/_sampler_ref.py against its fp64 restatement.

Batches of 1, 2, 3, 4, 5, 63, 64, 65 and 257 rows cut from the catalogue (one wave per row, 4 rows per block: the short
tail of the launch at every phase) and one of 65,536 + 261 different rows (the launch caps its grid at 16,384 blocks =
65,536 rows: the grid-stride loop runs, and a wrong row index shows).  Paths: uniforms given (0, 2^-24, 0.5, 1 - 2^-24,
1: the zero-mass prefix, the "rounding fell past the last mass" fallback), Philox with seed, step and env_offset below
2^32 and with a high word, deterministic, action_in (legal and illegal), NULL d_entropy / d_logp, and dstep with a base
at or above 2^32.  action, logp and entropy are written into sentinel-filled buffers whose outside stays untouched.

Bounds: actions by tests/test_gpu_ppo_kernels.py's rule (equal to the fp32 oracle's, or its target within K_ULP of a
CDF boundary); log-prob and entropy within the project's 1e-5 rtol / atol of the fp64 restatement (derivation:
_sampler_ref.RTOL).  Every check prints the kernel's and the fp32 oracle's worst errors before it asserts.  The empty
row returns action 0; its log-prob and entropy are NaN by construction and no reference sees it.
"""
import numpy as np
import pytest
import torch

import _sampler_ref as R
from oracle import bb_ppo as OP
from oracle import philox
from test_gpu_ppo_kernels import K_ULP, _check_sampled

pytestmark = pytest.mark.gpu

GUARD = 8
A_SENTINEL = -7777
F_SENTINEL = 12345.0
CAP_ROWS = 65536  # launch_masked_sample: 16,384 blocks of 4 rows
BIG = CAP_ROWS + 261
LOG_EPS32 = np.float32(np.log(np.float32(R.EPS32)))


@pytest.fixture(scope="module")
def rows():
    return R.corner_rows()


def _launch(dev, logits, mask, uniform=None, seed=0, step=0, env_offset=0, deterministic=False, action_in=None,
            want=("action", "logp", "entropy"), dstep_base=None):
    """One raw call -> {"action", "logp", "entropy"} numpy arrays (None where the pointer was NULL); each output is the
    inside of a larger buffer filled with a sentinel, whose outside is checked."""
    from runtime import kernels as K
    from runtime import lib as L

    lib, n = L.load(), logits.shape[0]
    lg = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev)
    mb = torch.from_numpy(R.mask_words(mask)).to(dev)
    bufs = {"action": torch.full((n + 2 * GUARD,), A_SENTINEL, dtype=torch.int64, device=dev),
            "logp": torch.full((n + 2 * GUARD,), F_SENTINEL, dtype=torch.float32, device=dev),
            "entropy": torch.full((n + 2 * GUARD,), F_SENTINEL, dtype=torch.float32, device=dev)}
    ptr = {k: (K._p(b[GUARD:]) if k in want else None) for k, b in bufs.items()}
    if dstep_base is not None:
        base = torch.tensor([dstep_base], dtype=torch.int64, device=dev)
        L.check(lib.bb_masked_sample_dstep(K._p(lg), K._p(mb), n, seed, K._p(base), step, env_offset,
                                           int(deterministic), ptr["action"], ptr["logp"], ptr["entropy"], K._s(dev)),
                "bb_masked_sample_dstep")
    else:
        u = None if uniform is None else torch.from_numpy(np.ascontiguousarray(uniform, np.float32)).to(dev)
        ai = None if action_in is None else torch.from_numpy(np.ascontiguousarray(action_in, np.int64)).to(dev)
        L.check(lib.bb_masked_sample(K._p(lg), K._p(mb), n, K._p(u), seed, step, env_offset, int(deterministic),
                                     K._p(ai), ptr["action"], ptr["logp"], ptr["entropy"], K._s(dev)),
                "bb_masked_sample")
    torch.cuda.synchronize(dev)
    out = {}
    for k, b in bufs.items():
        s = A_SENTINEL if k == "action" else F_SENTINEL
        assert bool((b[:GUARD] == s).all()) and bool((b[n + GUARD:] == s).all()), f"written outside {k}[0, n)"
        if k in want:
            out[k] = b[GUARD:n + GUARD].cpu().numpy()
        else:
            assert bool((b == s).all()), f"{k} written through a NULL pointer's neighbour"
            out[k] = None
    return out


def _check_fp64(label, logits, mask, action, lp, ent):
    """Log-prob and entropy of the non-empty rows at ``action`` against fp64; the fp32 oracle's errors beside them."""
    full = mask.any(axis=1)
    lg, mk, a = logits[full], mask[full], np.asarray(action)[full]
    _, lp32, ent32 = OP.masked_categorical(lg, mk, action=a)
    ol = R.errors(lp32, ent32, lg, mk, a)
    kl = R.errors(lp[full] if lp is not None else lp32, ent[full] if ent is not None else ent32, lg, mk, a)
    print(f"\n{label}: {int(full.sum())} rows; |err| against fp64 -- kernel logp {kl[2]:.2e} entropy {kl[3]:.2e} "
          f"({max(kl[:2]):.3f} of the bound); torch fp32 logp {ol[2]:.2e} entropy {ol[3]:.2e} ({max(ol[:2]):.3f})")
    if lp is not None:
        assert np.isfinite(lp[full]).all() and kl[0] <= 1.0, (label, "logp", kl)
    if ent is not None:
        assert np.isfinite(ent[full]).all() and kl[1] <= 1.0, (label, "entropy", kl)


def _check_sampling(label, logits, mask, u, got):
    """A sampled batch: the empty rows give action 0; on the others the action rule and the fp64 bounds."""
    full = mask.any(axis=1)
    assert (got["action"][~full] == 0).all()
    lg, mk, uu = logits[full], mask[full], np.asarray(u, np.float64)[full]
    a_ref, _, _ = OP.masked_categorical(lg, mk, uniform=uu)
    _check_sampled(lg, mk, uu, got["action"][full], got["logp"][full], got["entropy"][full], a_ref)
    _check_fp64(label, logits, mask, got["action"], got["logp"], got["entropy"])


BATCHES = R.batches(R.corner_rows())


@pytest.mark.parametrize("n,start", BATCHES, ids=[f"n{n}" for n, _ in BATCHES])
def test_corner_rows_with_uniforms_given(cuda, rows, n, start):
    b = R.take(rows, n, start)
    got = _launch(cuda, b["logits"], b["mask"], uniform=b["u"])
    _check_sampling(f"uniforms n {n}", b["logits"], b["mask"], b["u"], got)
    a, kind, u = got["action"], b["kind"], b["u"]
    # the rows built for one answer
    for k in R.SINGLE_AT:
        assert (a[kind == f"single@{k}"] == k).all()
    assert (a[(kind == "lead0") & (u < 1)] == R.LEAD0_AT).all() and (a[(kind == "lead0") & (u == 1)] == 191).all()
    assert (a[(kind == "trail0") & (u < 1)] == R.TRAIL0_AT).all()
    tail = (kind == "trail0") & (u == 1)
    assert (a[tail] == R.TRAIL0_LAST).all() and (got["logp"][tail] == LOG_EPS32).all()
    assert (a[(kind == "spread") & (u == 1)] == 191).all()
    for k in np.unique(kind[np.char.startswith(kind, "equal")]):
        assert (a[(kind == k) & (u == 0)] == 0).all() and (a[(kind == k) & (u == 1)] == 191).all()


@pytest.mark.parametrize("n,start", BATCHES, ids=[f"n{n}" for n, _ in BATCHES])
def test_corner_rows_deterministic_and_given_actions(cuda, rows, n, start):
    b = R.take(rows, n, start)
    lg, mk, full = b["logits"], b["mask"], ~b["empty"]
    det = _launch(cuda, lg, mk, deterministic=True)
    assert (det["action"][~full] == 0).all()
    if full.any():
        a_det, _, _ = OP.masked_categorical(lg[full], mk[full], deterministic=True)
        assert np.array_equal(det["action"][full], a_det)
        assert (det["action"][b["kind"] == "tie2"] == R.TIE2_AT[0]).all()  # the lower of two equal maxima
        _check_fp64(f"deterministic n {n}", lg, mk, det["action"], det["logp"], det["entropy"])
    # action_in: the deterministic action, and on every other row that has one an illegal action (P_a = 0)
    given = det["action"].copy()
    illegal = np.zeros(n, bool)
    for i in range(0, n, 2):
        off = np.flatnonzero(~mk[i])
        if full[i] and off.size:
            given[i], illegal[i] = off[(7 * i) % off.size], True
    ev = _launch(cuda, lg, mk, action_in=given)
    assert np.array_equal(ev["action"], given)  # d_action gets the given actions
    assert (ev["logp"][illegal] == LOG_EPS32).all()
    same = full & ~illegal
    assert np.array_equal(ev["logp"][same].view(np.int32), det["logp"][same].view(np.int32))
    assert np.array_equal(ev["entropy"][full].view(np.int32), det["entropy"][full].view(np.int32))
    if full.any():
        _check_fp64(f"action_in n {n}", lg, mk, given, ev["logp"], ev["entropy"])
        _, lp32, _ = OP.masked_categorical(lg[full], mk[full], action=given[full])
        assert (lp32[illegal[full]] == LOG_EPS32).all()  # the oracle agrees
    # NULL outputs: the others are bit-identical and nothing else is written
    for want in (("action", "logp"), ("action", "entropy"), ("logp",), ("action",)):
        part = _launch(cuda, lg, mk, deterministic=True, want=want)
        for k in want:
            assert np.array_equal(part[k][full].view(np.int32 if k != "action" else np.int64),
                                  det[k][full].view(np.int32 if k != "action" else np.int64)), (want, k)


HI = 1 << 32
PHILOX = [(77, 5, 100), (3 * HI + 77, 5, 100), (77, 9 * HI + 5, 100), (77, 5, 2 * HI + 100),
          (0xFEDCBA9876543210, 0x8000000000000001, 0xFFFFFFFF00000000)]


@pytest.mark.parametrize("seed,step,off", PHILOX, ids=[f"{s:#x}-{t:#x}-{o:#x}" for s, t, o in PHILOX])
def test_philox_counters_with_high_words(cuda, rows, seed, step, off):
    b = R.take(rows, 257, 11)
    u = philox.sample_uniform(257, seed=seed, step=step, env_offset=off)
    got = _launch(cuda, b["logits"], b["mask"], seed=seed, step=step, env_offset=off)
    _check_sampling(f"philox {seed:#x} {step:#x} {off:#x}", b["logits"], b["mask"], u, got)
    if (seed, step, off) != PHILOX[0]:  # another stream than the all-low counters'
        u0 = philox.sample_uniform(257, *PHILOX[0])
        assert (u != u0).mean() > 0.99


@pytest.mark.parametrize("base,add", [(HI, 0), (HI + 11, 3), (5 * HI - 1, 2), (7, 5)])
def test_dstep_is_the_plain_call_at_base_plus_add(cuda, rows, base, add):
    b = R.take(rows, 65, 80)
    seed, off = 3 * HI + 9, HI + 17
    for det in (False, True):
        plain = _launch(cuda, b["logits"], b["mask"], seed=seed, step=base + add, env_offset=off, deterministic=det)
        dstep = _launch(cuda, b["logits"], b["mask"], seed=seed, step=add, env_offset=off, deterministic=det,
                        dstep_base=base)
        full = ~b["empty"]
        assert np.array_equal(plain["action"], dstep["action"])
        for k in ("logp", "entropy"):
            assert np.array_equal(plain[k][full].view(np.int32), dstep[k][full].view(np.int32)), k
    u = philox.sample_uniform(65, seed=seed, step=base + add, env_offset=off)
    got = _launch(cuda, b["logits"], b["mask"], seed=seed, step=add, env_offset=off, dstep_base=base)
    _check_sampling(f"dstep {base:#x}+{add}", b["logits"], b["mask"], u, got)
    part = _launch(cuda, b["logits"], b["mask"], seed=seed, step=add, env_offset=off, dstep_base=base,
                   want=("action", "logp"))
    assert np.array_equal(part["action"], got["action"])


@pytest.fixture(scope="module")
def big():
    return R.big_rows(BIG)


def test_above_the_grid_cap_every_row_is_its_own(cuda, big):
    """65,536 + 261 different rows with Philox uniforms: the first 300 and the last 561 rows against the oracle, every
    action legal, and the rows past the cap bit-identical to their own 261-row launch at env_offset = 65,536."""
    lg, mk = big
    seed, step = 2 * HI + 31, HI + 4
    got = _launch(cuda, lg, mk, seed=seed, step=step)
    assert mk[np.arange(BIG), got["action"]].all()
    assert np.isfinite(got["logp"]).all() and np.isfinite(got["entropy"]).all()
    u = philox.sample_uniform(BIG, seed=seed, step=step)
    for name, sl in (("first 300", slice(0, 300)), ("last 561", slice(BIG - 561, BIG))):
        part = {k: v[sl] for k, v in got.items()}
        _check_sampling(f"big batch, {name}", lg[sl], mk[sl], u[sl], part)
    tail = _launch(cuda, lg[CAP_ROWS:], mk[CAP_ROWS:], seed=seed, step=step, env_offset=CAP_ROWS)
    assert np.array_equal(tail["action"], got["action"][CAP_ROWS:])
    for k in ("logp", "entropy"):
        assert np.array_equal(tail[k].view(np.int32), got[k][CAP_ROWS:].view(np.int32)), k


def test_above_the_grid_cap_with_uniforms_given(cuda, big):
    """The same batch with a uniform per row (the edges 0 and 1 among them), deterministic, and with actions given."""
    lg, mk = big
    rng = np.random.default_rng(99)
    u = rng.random(BIG).astype(np.float32)
    u[::101], u[50::101] = 0.0, 1.0
    got = _launch(cuda, lg, mk, uniform=u)
    assert mk[np.arange(BIG), got["action"]].all()
    # the ends of the CDF on every such row, by K_ULP's rule: at u = 0 no more than K_ULP 2^-24 of the mass lies before
    # the action, at u = 1 no more than that after it (the last legal action, or one whose successors carry nothing:
    # the fp64 prefix sums of two lanes may differ in the last bit)
    for edge in (0.0, 1.0):
        i = np.flatnonzero(u == edge)
        P, _, _ = R.reference(lg[i], mk[i], got["action"][i])
        k, a = np.arange(192)[None, :], got["action"][i][:, None]
        out = np.where(k < a if edge == 0.0 else k > a, P, 0.0).sum(axis=1)
        assert i.size > 600 and (out <= K_ULP * 2.0 ** -24).all(), (edge, float(out.max()))
    det = _launch(cuda, lg, mk, deterministic=True)
    ev = _launch(cuda, lg, mk, action_in=got["action"])
    assert np.array_equal(ev["logp"].view(np.int32), got["logp"].view(np.int32))
    assert np.array_equal(ev["entropy"].view(np.int32), det["entropy"].view(np.int32))
    for name, sl in (("first 300", slice(0, 300)), ("last 561", slice(BIG - 561, BIG))):
        _check_sampling(f"big batch, uniforms, {name}", lg[sl], mk[sl], u[sl], {k: v[sl] for k, v in got.items()})
        a_det, _, _ = OP.masked_categorical(lg[sl], mk[sl], deterministic=True)
        assert np.array_equal(det["action"][sl], a_det)
        _check_fp64(f"big batch, deterministic, {name}", lg[sl], mk[sl], det["action"][sl], det["logp"][sl],
                    det["entropy"][sl])
