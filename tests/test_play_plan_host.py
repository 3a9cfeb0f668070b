"""A plan played to its leaf on the host backend (bb_play_plan_pos of libbbvec_host.so), on the CPU: against the oracle
env and tests/_plan_ref.py's ``plan_lines`` on plans of 0-3 plies (tests/_play_plan_ref.py; the dead, refill and
illegal status bits each occur there), each output alone between guard words, every refusal with one text from both
libraries, n == 0 and the Python argument rules.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _plan_ref as P
import _play_plan_ref as PP

ERR_ARG = -1
FAKE = 0x1000


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


def test_host_equals_the_oracle_env(host):
    from runtime import kernels as K

    c = PP.cases()
    board, hand, combo, plan = PP.tensors(c, "cpu")
    got = K.play_plan(board, hand, plan, combo)
    assert set(got) == set(K.PLAY_PLAN_OUTPUTS) and all(t.shape == (len(c["env"]),) for t in got.values())
    PP.check(c, got)
    assert (K.PLAY_PLIES, K.PLAY_DEAD, K.PLAY_REFILL, K.PLAY_ILLEGAL) == (PP.PLIES, PP.DEAD, PP.REFILL, PP.ILLEGAL)


def test_lines_and_score_are_the_sums_of_plan_lines(host):
    from runtime import kernels as K

    c = PP.cases()
    board, hand, combo, plan = PP.tensors(c, "cpu")
    got = K.play_plan(board, hand, plan, combo, want=("lines", "score", "status"))
    legal = np.nonzero((c["exp_status"] & PP.ILLEGAL) == 0)[0][::3]
    assert len(legal) >= 20
    for i in legal:
        lines, gained = P.plan_lines(c["board"][i], c["hand"][i], c["combo"][i], c["plan"][i].tolist())
        assert int(got["lines"][i]) == sum(lines) and int(got["score"][i]) == sum(gained), i
        assert int(got["status"][i]) & PP.PLIES == len(lines)


def test_no_combo_column_reads_as_zero(host):
    from runtime import kernels as K

    c = PP.cases()
    board, hand, _, plan = PP.tensors(c, "cpu")
    a = K.play_plan(board, hand, plan, None)
    b = K.play_plan(board, hand, plan, torch.zeros(len(board), dtype=torch.int32))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_each_output_alone_and_nothing_beyond_it(host):
    from runtime import lib as L

    c = PP.cases()
    n = len(c["env"])
    cols = {"board": np.uint64, "hand": np.uint32, "combo": np.int32, "lines": np.int32, "score": np.int64,
            "status": np.int32}
    bufs = {k: np.zeros(n + 16, dt) for k, dt in cols.items()}
    combo = c["combo"].astype(np.int32)
    pos = L.Positions(board=c["board"].ctypes.data, hand=c["hand"].ctypes.data, combo=combo.ctypes.data, prev=None)
    plan = np.ascontiguousarray(c["plan"])
    for wanted in [(k,) for k in cols] + [tuple(cols)]:
        for v in bufs.values():
            v[:] = 0x5A
        o = L.PlayPlanOut(**{k: bufs[k][8:].ctypes.data for k in wanted})
        assert host.bb_play_plan_pos(C.byref(pos), n, plan.ctypes.data, C.byref(o), None) == 0
        for k, v in bufs.items():
            assert (v[:8] == 0x5A).all() and (v[8 + n:] == 0x5A).all(), k
            if k in wanted:
                assert v[8:8 + n].astype(np.int64).tolist() == c["exp_" + k].astype(np.int64).tolist(), k
            else:
                assert (v == 0x5A).all(), k


_NO_POS = [dict(pos=None), dict(pos=dict(board=None, hand=FAKE)), dict(pos=dict(board=FAKE, hand=None))]
REFUSALS = ([(kw, "positions (board, hand) are NULL") for kw in _NO_POS]
            + [(dict(n=-1), "n is negative"), (dict(plan=None), "d_plan is NULL"), (dict(out=None), "out is NULL"),
               (dict(out={}), "all six outputs are NULL")])


def _call(backend, kw):
    from runtime import lib as L

    a = {"pos": dict(board=FAKE, hand=FAKE), "n": 4, "plan": FAKE, "out": dict(status=FAKE), **kw}
    pos = L.Positions(**a["pos"]) if a["pos"] is not None else None
    o = L.PlayPlanOut(**a["out"]) if a["out"] is not None else None
    return backend.bb_play_plan_pos(C.byref(pos) if pos is not None else None, a["n"], a["plan"],
                                    C.byref(o) if o is not None else None, None)


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[f"{i}-{t}" for i, (_, t) in enumerate(REFUSALS)])
def test_rules_are_one_set_for_both_backends(lib, host, kw, text):
    """Refused with BB_ERR_ARG before any HIP call (so libbbvec.so answers without a GPU), the same text from both."""
    from runtime import lib as L

    for backend in (lib, host):
        assert _call(backend, kw) == ERR_ARG
        assert L.last_error(lib=backend) == f"bb_play_plan_pos: {text}"


def test_no_positions_is_accepted_and_does_nothing(lib, host):
    from runtime import kernels as K

    for backend in (lib, host):
        assert _call(backend, dict(n=0)) == 0
    got = K.play_plan(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                      torch.zeros((0, 3), dtype=torch.int32))
    assert set(got) == set(K.PLAY_PLAN_OUTPUTS) and all(t.shape == (0,) for t in got.values())


def test_python_argument_rules(host):
    from runtime import kernels as K
    from runtime import lib as L

    c = PP.cases()
    board, hand, combo, plan = (t[:6].contiguous() for t in PP.tensors(c, "cpu"))
    with pytest.raises(L.BBNativeError, match="board must be a contiguous"):
        K.play_plan(board.to(torch.int32), hand, plan)
    with pytest.raises(L.BBNativeError, match="hand must be a contiguous"):
        K.play_plan(board, hand[:5], plan)
    with pytest.raises(L.BBNativeError, match="combo must be a contiguous"):
        K.play_plan(board, hand, plan, combo.long())
    for bad in (plan.long(), plan[:5], plan.reshape(-1), torch.zeros((6, 6), dtype=torch.int32)[:, ::2]):
        with pytest.raises(L.BBNativeError, match="plan must be a contiguous"):
            K.play_plan(board, hand, bad)
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.play_plan(board, hand, plan, want=("board", "value"))
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.play_plan(board, hand, plan, out={"value": torch.zeros(6, dtype=torch.int64)})
    with pytest.raises(L.BBNativeError, match="at least one of"):
        K.play_plan(board, hand, plan, out={})
    with pytest.raises(L.BBNativeError, match="score must be a contiguous"):
        K.play_plan(board, hand, plan, out={"score": torch.zeros(6, dtype=torch.int32)})
    out = {"status": torch.zeros(6, dtype=torch.int32)}
    assert K.play_plan(board, hand, plan, combo, out=out) is out
    assert out["status"].tolist() == c["exp_status"][:6].tolist()
