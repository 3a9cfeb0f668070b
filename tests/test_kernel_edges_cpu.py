"""The sampler's corner rows (tests/_sampler_ref.py) without a GPU: the fp32 torch oracle
(oracle.bb_ppo.masked_categorical) meets the GPU tests' bounds against the fp64 restatement on every non-empty row --
the inputs are fair to an fp32 implementation -- and returns the actions the rows were built for; and the catalogue and
the batches cut from it exercise every kind.  Likewise for BatchNorm: the fp64 restatement of tests/_bn_ref.py is
torch's float64 module, its case list exercises every channel kind, shape, layout and dtype, and
bb_bn_workspace_bytes (host-only code of libbbvec.so) keeps to the NCHW row limit of include/bbvec.h.
"""
import numpy as np
import pytest

import _sampler_ref as R
from oracle import bb_ppo as OP


@pytest.fixture(scope="module")
def rows():
    return R.corner_rows()


@pytest.fixture(scope="module")
def oracle(rows):
    """The fp32 oracle on the non-empty rows: sampled with the rows' uniforms, and deterministic."""
    full = ~rows["empty"]
    lg, mk, u = rows["logits"][full], rows["mask"][full], rows["u"][full]
    a, lp, ent = OP.masked_categorical(lg, mk, uniform=u.astype(np.float64))
    det, lpd, _ = OP.masked_categorical(lg, mk, deterministic=True)
    return {"rows": np.flatnonzero(full), "a": a, "lp": lp, "ent": ent, "det": det, "lp_det": lpd}


def _at(rows, oracle, kind, u=None):
    """Positions in the oracle's arrays of the rows of ``kind`` (at uniform ``u``)."""
    sel = rows["kind"][oracle["rows"]] == kind
    if u is not None:
        sel &= rows["u"][oracle["rows"]] == np.float32(u)
    return np.flatnonzero(sel)


def test_fp32_oracle_meets_the_bounds_against_fp64(rows, oracle):
    i = oracle["rows"]
    lg, mk = rows["logits"][i], rows["mask"][i]
    assert np.isfinite(oracle["lp"]).all() and np.isfinite(oracle["ent"]).all()
    for a, lp in ((oracle["a"], oracle["lp"]), (oracle["det"], oracle["lp_det"])):
        assert mk[np.arange(i.size), a].all()
        rl, re, al, ae = R.errors(lp, oracle["ent"], lg, mk, a)
        print(f"torch fp32 against fp64 on {i.size} corner rows: logp {al:.2e} ({rl:.3f} of the bound), "
              f"entropy {ae:.2e} ({re:.3f})")
        assert rl <= 1.0 and re <= 1.0
    # an illegal action given: P_a = 0, the log-prob is log(eps32) on both sides
    illegal = np.array([int(np.flatnonzero(~m)[0]) if not m.all() else -1 for m in mk])
    has = illegal >= 0
    _, lp, ent = OP.masked_categorical(lg[has], mk[has], action=illegal[has])
    assert (lp == np.float32(np.log(np.float32(R.EPS32)))).all()
    assert R.errors(lp, ent, lg[has], mk[has], illegal[has])[0] <= 1.0


def test_oracle_actions_on_the_corner_rows(rows, oracle):
    a, det = oracle["a"], oracle["det"]
    for k in R.SINGLE_AT:
        assert (a[_at(rows, oracle, f"single@{k}")] == k).all() and (det[_at(rows, oracle, f"single@{k}")] == k).all()
    assert (a[_at(rows, oracle, "lead0")][:4] == R.LEAD0_AT).all()  # u = 0 skips the zero-mass prefix
    assert a[_at(rows, oracle, "lead0", 1.0)] == 191  # the fallback again
    assert a[_at(rows, oracle, "trail0", 0.0)] == R.TRAIL0_AT
    assert a[_at(rows, oracle, "trail0", 1.0)] == R.TRAIL0_LAST  # the fallback: the last legal action
    assert oracle["lp"][_at(rows, oracle, "trail0", 1.0)] == np.float32(np.log(np.float32(R.EPS32)))
    assert a[_at(rows, oracle, "spread", 1.0)] == 191
    assert (det[_at(rows, oracle, "tie2")] == R.TIE2_AT[0]).all()  # the lower of the two maxima
    for v in R.EQUAL_VALUES:
        k = f"equal:{v:g}"
        assert a[_at(rows, oracle, k, 0.0)] == 0 and a[_at(rows, oracle, k, 1.0)] == 191
        assert a[_at(rows, oracle, k, 0.5)] in (95, 96) and a[_at(rows, oracle, k, R.U_THIRD)] in (63, 64)
        assert (det[_at(rows, oracle, k)] == 0).all()


def test_rows_exercise_every_kind(rows, oracle):
    kinds = rows["kind"]
    names = ([f"single@{k}" for k in R.SINGLE_AT] + [f"equal:{v:g}" for v in R.EQUAL_VALUES]
             + ["tie2", "spread", "lead0", "trail0", "empty"]
             + [f"random:{d}:{s:g}" for d in ("one", "tenth", "all") for s in (1.0, 30.0)])
    assert sorted(set(kinds.tolist())) == sorted(names)
    for k in names:  # every kind at every uniform, `equal` at 1/3 too
        us = sorted(rows["u"][kinds == k].tolist())
        want = sorted(float(u) for u in R.U_EDGES + ((R.U_THIRD,) if k.startswith("equal") else ()))
        assert us == want, k
    mk, lg = rows["mask"], rows["logits"]
    count = lambda k: set(mk[kinds == k].sum(axis=1).tolist())  # noqa: E731
    for k in R.SINGLE_AT:
        assert count(f"single@{k}") == {1} and mk[kinds == f"single@{k}"][:, k].all()
        assert k % 64 in (0, 63)  # a word edge
    assert count("empty") == {0} and count("random:one:1") == {1} and count("random:all:30") == {192}
    assert all(5 <= c <= 40 for c in count("random:tenth:1") | count("random:tenth:30"))
    for v in R.EQUAL_VALUES:
        assert (lg[kinds == f"equal:{v:g}"] == np.float32(v)).all() and np.isfinite(np.float32(v))
    # tie2: the two maxima are equal, legal, and in different words
    t = np.flatnonzero(kinds == "tie2")[0]
    top = np.flatnonzero(mk[t] & (lg[t] == lg[t][mk[t]].max()))
    assert top.tolist() == list(R.TIE2_AT) and top[0] // 64 != top[1] // 64
    # spread: in fp32 every probability but the maximum underflows to 0; the last legal action is not the maximum
    s = np.flatnonzero(kinds == "spread")[0]
    legal = np.sort(lg[s][mk[s]])
    assert 70 <= mk[s].sum() <= 125 and legal[-1] - legal[-2] > 150.0 and mk[s][191] and lg[s][191] < legal[-1]
    # lead0 / trail0: a zero-mass prefix before, and a zero-mass legal tail after, the only mass
    P, _, _ = R.reference(lg[kinds == "lead0"][:1], mk[kinds == "lead0"][:1], [R.LEAD0_AT])
    assert np.float32(P[0, :R.LEAD0_AT].sum()) == 0 and np.float32(np.exp(np.float32(-200.0))) == 0
    tm = mk[kinds == "trail0"][0]
    assert tm[:R.TRAIL0_LAST + 1].all() and not tm[R.TRAIL0_LAST + 1:].any() and R.TRAIL0_AT < R.TRAIL0_LAST
    # the uniforms reach both ends: u = 1 takes the fallback (no CDF entry above the target) on every non-empty row
    i = oracle["rows"][rows["u"][oracle["rows"]] == np.float32(1.0)]
    cdf = OP.categorical_cdf(lg[i], mk[i])
    assert not (cdf > cdf[:, -1:]).any()
    assert float(R.U_EDGES[3]) < 1.0 and float(R.U_EDGES[1]) > 0.0


def test_batches_cover_the_catalogue(rows):
    sizes = [n for n, _ in R.batches(rows)]
    assert sizes == [1, 2, 3, 4, 5, 63, 64, 65, 257]
    seen = set()
    inner_empty = False
    for n, start in R.batches(rows):
        b = R.take(rows, n, start)
        seen |= set(b["idx"].tolist())
        e = np.flatnonzero(b["empty"])
        inner_empty |= bool(((e > 0) & (e < n - 1)).any()) and not b["empty"].all()
        if n > 1:
            assert not b["empty"].all()
    assert seen == set(range(len(rows["kind"]))) and inner_empty
    one = R.take(rows, *R.batches(rows)[0])
    assert one["kind"][0] == "trail0" and one["u"][0] == np.float32(1.0)
    for n in (2, 3):  # the empty row beside a non-empty neighbour in the shortest launches
        b = R.take(rows, *[x for x in R.batches(rows) if x[0] == n][0])
        assert b["empty"].any() and not b["empty"].all()


def test_reference_refuses_an_empty_row(rows):
    e = np.flatnonzero(rows["empty"])[:1]
    with pytest.raises(AssertionError):
        R.reference(rows["logits"][e], rows["mask"][e], [0])


def test_big_rows_are_all_different():
    lg, mk = R.big_rows(65536 + 261)
    key = np.ascontiguousarray(lg[:, :2]).view(np.uint64)[:, 0]
    assert np.unique(key).size == lg.shape[0] and mk.any(axis=1).all()


# ---------------------------------------------------------------------------------------------------------------
# bb_bn_workspace_bytes: an NCHW row is at most 256 16-byte vectors (include/bbvec.h).  The launch plan's
# rows-per-iteration is 256 / (vectors per row): beyond the limit it was 0 and the next line divided by it.
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,hw,ok", [(0, 4096, False), (1, 4096, False), (0, 1024, True), (1, 2048, True),
                                         (0, 1028, False), (1, 2056, False)])
def test_bn_workspace_bytes_nchw_row_limit(lib, dtype, hw, ok):
    nbytes = lib.bb_bn_workspace_bytes(dtype, 0, 4, 8, hw)
    assert (nbytes > 0) if ok else (nbytes == -1)
    if not ok:
        from runtime import lib as L

        assert "256 16-byte vectors" in L.last_error()


# ---------------------------------------------------------------------------------------------------------------
# tests/_bn_ref.py: the fp64 BatchNorm restatement against torch's float64 module on the CPU, and the case list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu,pre_bias", [(False, False), (True, True)])
def test_bn_reference_is_torch_float64(relu, pre_bias):
    import torch

    import _bn_ref as B

    case = B.Case(5, 6, 4, False, False, relu, pre_bias, 0.25, 3)
    inp = B.inputs(case)
    ref = B.reference(inp["x"], inp["dy"], inp["weight"], inp["bias"], inp["pre_bias"], inp["running_mean"],
                      inp["running_var"], 0.25, 1e-5, relu)
    m = torch.nn.BatchNorm2d(6, eps=1e-5, momentum=0.25).double().train()
    with torch.no_grad():
        for p, k in ((m.weight, "weight"), (m.bias, "bias"), (m.running_mean, "running_mean"),
                     (m.running_var, "running_var")):
            p.copy_(torch.from_numpy(inp[k]))
    x = torch.from_numpy(inp["x"]).requires_grad_(True)
    pb = torch.from_numpy(inp["pre_bias"]).requires_grad_(True) if pre_bias else None
    y = m(x + pb.view(1, -1, 1, 1) if pre_bias else x)
    y = torch.relu(y) if relu else y
    y.backward(torch.from_numpy(inp["dy"]))
    want = {"y": y, "running_mean": m.running_mean, "running_var": m.running_var, "dx": x.grad,
            "dweight": m.weight.grad, "dbias": m.bias.grad, "dpre_bias": pb.grad if pre_bias else None}
    for k, v in want.items():
        if v is not None:
            np.testing.assert_allclose(ref[k], v.detach().numpy(), rtol=1e-9, atol=1e-9, err_msg=k)
    assert (ref["abs_dweight"] >= np.abs(ref["dweight"])).all() and (ref["abs_dbias"] >= np.abs(ref["dbias"])).all()
    if relu:  # the dead channel: every output 0
        d = inp["kinds"] == "dead"
        assert d.any() and not ref["y"][:, d].any() and not ref["dx"][:, d].any() and not ref["dweight"][d].any()


def test_bn_cases_exercise_every_kind_and_shape():
    import _bn_ref as B

    cases = B.cases()
    assert len(set(B.case_id(k) for k in cases)) == len(cases)
    for nhwc in (False, True):
        for bf16 in (False, True):
            mine = [k for k in cases if k.nhwc == nhwc and k.bf16 == bf16]
            assert {k.n for k in mine if k.h == 8} == {1, 3, 33, 257}
            assert {k.c for k in mine} >= ({8, 64, 128} if nhwc and bf16 else {4, 8, 64, 128})
            assert {(k.relu, k.pre_bias) for k in mine if k.h == 8} == {(a, b) for a in (0, 1) for b in (0, 1)}
            assert {k.momentum for k in mine} == {0.1, 0.25}
            seen = set()
            for k in mine:
                assert B.fusable(k.c, k.h, k.nhwc, k.bf16)
                seen |= {(kind, k.relu) for kind in B.kinds_of(k).tolist()}
            assert seen >= {(kind, r) for kind in B.KINDS[:-1] for r in (False, True)} | {("dead", True)}
            assert ("dead", False) not in seen
    assert {k.h for k in cases if not k.nhwc and not k.bf16} == {2, 4, 6, 8, 16, 32}
    assert {k.h for k in cases if not k.nhwc and k.bf16} == {4, 8, 16, 32}
    assert not B.fusable(8, 64, False, False) and not B.fusable(8, 64, False, True)
    # the kinds are what they are named for
    inp = B.inputs(B.Case(33, 6, 8, False, False, True, False, 0.1, 0))
    x, kinds = inp["x"], inp["kinds"]
    assert kinds.tolist() == list(B.KINDS)
    std, mean = x.std(axis=(0, 2, 3)), x.mean(axis=(0, 2, 3))
    assert std[2] == 0 and mean[2] == 0.5 and std[3] ** 2 < 0.2 * 1e-5 and std[4] > 900
    assert abs(mean[1]) > 25 * std[1] and inp["weight"][5] == 0.01 and inp["bias"][5] == -5.0
