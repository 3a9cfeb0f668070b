"""bb_plan2_values(_pos) on the host backend (CPU) against tests/_plan2_ref.py: the oracle restatement, which calls no
entry point of the library for its values, at depth 1-3, and the composition of the existing entry points on the whole
position set.  Integer-exact, all five outputs."""
import numpy as np
import pytest
import torch

import _plan2_ref as P2

INT64_MIN = P2.INT64_MIN
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def pos(host):
    board, hand, combo, names = P2.positions()
    return {"np": (board, hand, combo), "t": P2.to_tensors(board, hand, combo, CPU), "names": names,
            "n": len(board), "rows": P2.mixed_rows(len(board), CPU)}


@pytest.mark.parametrize("depth", [1, 2])
def test_the_oracle_restatement_with_a_row_and_a_stream_each(host, pos, depth):
    from runtime import kernels as K

    board, hand, combo = pos["np"]
    names = pos["names"]
    sel = [3, 31, 47, 60, 95, 120, names["one_slot_left"], names["combo5_row_short"], names["game_over_bit"],
           names["col_short"]]
    ws = [P2.SHAPED, P2.PLAIN] * 5
    stream = [4, 4, 9, 1, 0, 2, 2, 7, 7, 3]
    want = P2.oracle(board[sel], hand[sel], combo[sel], ws, depth, 3, 2, 77, stream=stream)
    got = P2.call(*P2.to_tensors(board, hand, combo, CPU, sel), torch.cat([K.eval_rows(w) for w in ws]), depth, 3, 2,
                  77, stream=torch.tensor(stream, dtype=torch.int64))
    P2.assert_equal(got, want, f"depth {depth}")
    assert P2.leaf_kinds(want)[0] >= 9 and (want["status"] == -1).any()


def test_the_oracle_restatement_at_depth_3(host, pos):
    from runtime import kernels as K

    board, hand, combo = pos["np"]
    sel = [20]  # one mid-game position, one candidate, one deal: a dealt hand searched three plies deep is dear
    want = P2.oracle(board[sel], hand[sel], combo[sel], P2.SHAPED, 3, 1, 1, 5)
    got = P2.call(*P2.to_tensors(board, hand, combo, CPU, sel), K.eval_rows(P2.SHAPED), 3, 1, 1, 5)
    P2.assert_equal(got, want, "depth 3")
    assert P2.leaf_kinds(want)[0] == 1 and want["value"].any()


@pytest.mark.parametrize("depth,k,deals", [(1, 192, 1), (2, 8, 3), (3, 3, 2)])
def test_the_position_set_against_the_composed_entry_points(host, pos, depth, k, deals):
    n, names = pos["n"], pos["names"]
    stream = (torch.arange(n) // 2).to(torch.int64)
    want = P2.as_numpy(P2.composed(*pos["t"], pos["rows"], depth, k, deals, 3, stream=stream))
    got = P2.call(*pos["t"], pos["rows"], depth, k, deals, 3, stream=stream)
    P2.assert_equal(got, want, f"depth {depth}")
    refill, dead, cut = P2.leaf_kinds(want)
    assert refill > 20 and dead > 10 and (cut > 20 or depth == 3)
    is_refill = (want["status"] >= 0) & ((want["status"] & 8) != 0)
    assert not want["value"][~is_refill].any()
    for name in ("game_over_bit", "all_used", "full_but_one"):
        i = names[name]
        assert got["action"][i] == 0 and (got["q2"][i] == INT64_MIN).all() and (got["cand"][i] == -1).all()
    if depth == 1:
        assert (want["cand"][names["empty_singles"]] >= 0).all()  # 192 candidates


def test_zero_shape_rows_are_the_eight_weight_calls_and_ties_go_to_the_lower_action(host, pos):
    from agents.greedy import TwoHandPlanAgent
    from runtime import kernels as K

    tb, th, tc = pos["t"]
    got = P2.call(tb, th, tc, K.eval_rows(P2.PLAIN), 2, 4, 3, TwoHandPlanAgent.deal_seed(9, 0), want=("action",))
    agent = TwoHandPlanAgent(P2.R.DEFAULT_WEIGHTS, depth=2, candidates=4, deals=3, seed=9, device="cpu")
    pv = K.plan_values(tb, th, P2.R.DEFAULT_WEIGHTS, 2, combo=tc, want=("q", "rest"))
    assert torch.equal(got["action"].long(), agent._decide(tb, th, tc, pv["q"], pv["rest"]))
    rows = K.eval_rows({**P2.ZERO12, "lines": 1})
    want = P2.as_numpy(P2.composed(tb, th, tc, rows, 1, 4, 1, 2))
    got = P2.call(tb, th, tc, rows, 1, 4, 1, 2)
    P2.assert_equal(got, want, "rank order")
    i = pos["names"]["col_short"]  # the first-ranked candidate ties with a lower action: the lower action wins
    assert want["cand"][i].tolist() == [184, 129, 130, 131] and want["q2"][i, 184] == want["q2"][i, 129] == 1
    assert got["action"][i] == 129


def test_each_output_alone_between_guard_words_and_the_size_query(host, pos):
    from runtime import kernels as K
    from runtime import lib as L

    tb, th, tc = (t[:40].contiguous() for t in pos["t"])
    rows = pos["rows"][:40].contiguous()
    k, deals = 5, 3
    want = P2.call(tb, th, tc, rows, 2, k, deals, 13)
    need = K.plan2_work_bytes(40, k, deals, host=True)
    assert need == 40 * (192 * 12 + k * 28 + k * deals * 8) and host.bb_plan2_work_bytes(0, 1, 1) == 0
    assert host.bb_plan2_work_bytes(3, 1, 1) == (3 * (192 * 12 + 28 + 8) + 7) // 8 * 8
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 193, 1), (1, 1, 0), (1, 1, 1025)):
        assert host.bb_plan2_work_bytes(*bad) < 0
    work = torch.full((need + 128,), 0x5A, dtype=torch.uint8)
    for key in P2.OUTPUTS:
        buf, view = P2.guarded(40, k, deals, CPU, key)
        P2.call(tb, th, tc, rows, 2, k, deals, 13, out={key: view}, work=work[64:64 + need])
        assert torch.equal(view, want[key]) and P2.guards_intact(buf) and P2.guards_intact(work), key
    with pytest.raises(L.BBNativeError, match="work has"):
        P2.call(tb, th, tc, rows, 2, k, deals, 13, work=work[64:64 + need - 8])
    for kw, text in ((dict(k=0), "candidates must be 1..192"), (dict(deals=1025), "deals must be 1..1024"),
                     (dict(depth=4), "depth must be 1..3")):
        a = {**dict(depth=2, k=k, deals=deals), **kw}
        with pytest.raises(L.BBNativeError, match=text):
            P2.call(tb, th, tc, rows, a["depth"], a["k"], a["deals"], 13)
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        P2.call(tb, th, tc, rows, 2, k, deals, 13, want=("action", "plan"))
    with pytest.raises(L.BBNativeError, match="rows must be"):
        P2.call(tb, th, tc, rows[:7], 2, k, deals, 13)
