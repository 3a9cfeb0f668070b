"""bb_adam_clip_step (csrc/bb_optim.hip) at its edges against the fp64 restatement of tests/_optim_ref.py.

Every case of the catalogue (every size around a 2,048-element chunk, every alignment variant -- so the norm kernel
and the update kernel take their scalar and float4 paths together and apart -- a table of exactly 48 tensors, chunk
totals around the finaliser's 8-wide loop, non-zero moments at steps 9 .. 99999, zero / mixed-magnitude / unclipped
gradients) runs three chained steps through K.adam_clip_step on views into guarded flat buffers.  Each step starts
from the kernel's own previous outputs and is compared with the restatement run from those same values, so no error
carries over.  After each step:

  norm        |total_norm - norm64| <= 6 u norm64, u = 2^-24.  A thread sums at most 8 fp32 squares (each product one
              rounding, seven adds: the sum within 8 u of exact) and everything above is fp64; the root halves that
              to 4 u and the rounding of the result to fp32 adds 1 u.
  g'          bit for bit the replay's fl32(g coef32): one IEEE fp32 product, coef32 from the reported norm in fp32
              arithmetic (an IEEE divide).  Where coef32 == 1, bit for bit the input.
  m', v'      within 1 fp32 ulp of the replay, and off the replay on at most 1e-4 of the case's elements: the kernel
              forms them in fp64 from fp32 operands and rounds once, as the replay does; double rounding or a
              contraction can flip that rounding only within about 2^-28 of a tie, while fp32 moment arithmetic or
              truncation would differ on a large share.
  p'          |p - p'replay| <= 8 u |upd64| + u |p'|: about five fp32 roundings sit in the step size, the root, the
              two divisions and the product (and a 1-ulp moment costs 2 u), half an ulp of p' in the subtraction.
  step        prior + 1 exactly.
  guards      every float between and around the views of all four flat buffers still holds its sentinel, and the
              finaliser's guard word is clean (adam_guard_check).
"""
import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

CASES = R.adam_cases()


def run_case(case, cuda, step_fn, steps=3):
    """Three chained steps of ``step_fn(views p, g, m, v, step tensors, max_norm) -> fp32 norm`` on the case's guarded
    buffers -> list per step of (ratios of R.measure, step counts ok, guards ok)."""
    b = R.build(case)
    st, tot, sz = b["starts"], b["totals"], case.sizes
    dev = {k: torch.from_numpy(b["flat"][k]).to(cuda) for k in "pmv"}
    dev["g"] = torch.empty(tot[1], dtype=torch.float32, device=cuda)
    steps_dev = [torch.full((), s, dtype=torch.float32, device=cuda) for s in b["steps"]]
    tv = {k: [dev[k][s:s + n] for s, n in zip(st["pgmv".index(k)], sz)] for k in "pgmv"}
    for k in "pgmv":
        assert [t.data_ptr() % 16 // 4 for t in tv[k]] == [R.ALIGNS[a]["pgmv".index(k)] for a in case.aligns]
    host = {k: b["flat"][k] for k in "pmv"}
    prior = list(b["steps"])
    out = []
    for k in range(steps):
        host["g"] = R.flat_gradients(case, k, st, tot)
        dev["g"].copy_(torch.from_numpy(host["g"]))
        before = {q: R.views(host[q], st["pgmv".index(q)], sz) for q in "pgmv"}
        norm = step_fn(tv["p"], tv["g"], tv["m"], tv["v"], steps_dev, case.max_norm)
        after_flat = {q: dev[q].cpu().numpy() for q in "pgmv"}
        got = {q: R.views(after_flat[q], st["pgmv".index(q)], sz) for q in "pgmv"}
        got["norm"] = np.float32(norm)
        ref = R.adam_clip_ref(before["p"], before["g"], before["m"], before["v"], prior, R.LR, R.BETA1, R.BETA2,
                              R.EPS, case.max_norm, got["norm"])
        ratios = R.measure(got, ref, ref["coef"] == 1.0, before["g"])
        steps_ok = [float(s) for s in steps_dev] == ref["step"]
        guards_ok = all(R.guards_intact(after_flat[q], st["pgmv".index(q)], sz) for q in "pgmv")
        out.append((ratios, steps_ok, guards_ok))
        host, prior = after_flat, ref["step"]
    return out


def ours(cuda, sizes):
    from runtime import kernels as K

    ws = K.adam_clip_workspace(list(sizes), cuda)
    norm = torch.zeros((), device=cuda)

    def step(p, g, m, v, steps, max_norm):
        K.adam_clip_step(p, g, m, v, steps, R.LR, R.BETA1, R.BETA2, R.EPS, max_norm, ws, norm)
        return float(norm)

    return step, ws


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_adam_clip_step_meets_the_fp64_bounds(cuda, case):
    from runtime import kernels as K

    step, ws = ours(cuda, case.sizes)
    for k, (r, steps_ok, guards_ok) in enumerate(run_case(case, cuda, step)):
        print(f"{case.name} step {k}: " + ", ".join(f"{n} {v:.3g}" for n, v in r.items()))
        assert r["norm"] <= 1.0, (k, r)
        assert r["g_bits"] == 0.0, (k, "clipped gradient differs from fl32(g * coef32)")
        assert r["m_ulp"] <= 1.0 and r["v_ulp"] <= 1.0, (k, r)
        assert r["m_share"] <= 1.0 and r["v_share"] <= 1.0, (k, r)
        assert r["p"] <= 1.0, (k, r)
        assert steps_ok, k
        assert guards_ok, (k, "a guard float next to a view was written")
    K.adam_guard_check(ws, list(case.sizes))


def test_adam_clip_step_is_deterministic_at_the_table_limit_and_mixed_alignment(cuda):
    by = {c.name: c for c in CASES}
    for name in ("table48", "mixed-align"):
        case = by[name]
        runs = []
        for _ in range(2):
            b = R.build(case)
            st, tot, sz = b["starts"], b["totals"], case.sizes
            dev = {k: torch.from_numpy(b["flat"][k]).to(cuda) for k in "pmv"}
            dev["g"] = torch.empty(tot[1], dtype=torch.float32, device=cuda)
            tv = {k: [dev[k][s:s + n] for s, n in zip(st["pgmv".index(k)], sz)] for k in "pgmv"}
            steps_dev = [torch.full((), s, dtype=torch.float32, device=cuda) for s in b["steps"]]
            step, _ = ours(cuda, sz)
            norms = []
            for k in range(3):
                dev["g"].copy_(torch.from_numpy(R.flat_gradients(case, k, st, tot)))
                norms.append(step(tv["p"], tv["g"], tv["m"], tv["v"], steps_dev, case.max_norm))
            runs.append([dev[k].clone() for k in "pgmv"] + [torch.tensor(norms)])
        for a, c in zip(*runs):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), name
