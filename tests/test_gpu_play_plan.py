"""A plan played to its leaf on the MI355X (bb_play_plan_pos of libbbvec.so, play_plan_kernel in
csrc/bb_lookahead.hip): HIP = the host backend = the oracle env on the plans of tests/_play_plan_ref.py (0-3 plies;
dead, refill and illegal leaves), the cases tiled past one workgroup, each output alone between guard words, and
tensors on the wrong side refused.
"""
import pytest
import torch

import _play_plan_ref as PP

pytestmark = pytest.mark.gpu

FILL = -7


def test_hip_equals_the_host_backend_and_the_oracle_env(cuda):
    from runtime import kernels as K

    c = PP.cases()
    cpu = PP.tensors(c, "cpu")
    board, hand, combo, plan = PP.tensors(c, cuda)
    got = K.play_plan(board, hand, plan, combo)
    want = K.play_plan(cpu[0], cpu[1], cpu[3], cpu[2])
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k
    PP.check(c, got)
    nocombo = K.play_plan(board, hand, plan, None, want=("score", "combo"))
    host = K.play_plan(cpu[0], cpu[1], cpu[3], None, want=("score", "combo"))
    assert torch.equal(nocombo["score"].cpu(), host["score"]) and torch.equal(nocombo["combo"].cpu(), host["combo"])


def test_more_positions_than_one_workgroup(cuda):
    """The cases tiled to 5 * 256 + 3 positions, shifted by one per tile so that a lane meets another piece."""
    from runtime import kernels as K

    c = PP.cases()
    n = 5 * 256 + 3
    idx = (torch.arange(n) + torch.arange(n) // len(c["env"])) % len(c["env"])
    cpu = [t[idx].contiguous() for t in PP.tensors(c, "cpu")]
    want = K.play_plan(cpu[0], cpu[1], cpu[3], cpu[2])
    got = K.play_plan(cpu[0].to(cuda), cpu[1].to(cuda), cpu[3].to(cuda), cpu[2].to(cuda))
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k


@pytest.mark.parametrize("wanted", [("board",), ("hand",), ("combo",), ("lines",), ("score",), ("status",),
                                    ("board", "hand", "combo", "lines", "score", "status")],
                         ids=["board", "hand", "combo", "lines", "score", "status", "all"])
def test_each_output_alone_between_guard_words(cuda, wanted):
    from runtime import kernels as K

    c = PP.cases()
    n = len(c["env"])
    board, hand, combo, plan = PP.tensors(c, cuda)
    bufs = {k: torch.full((n + 16,), FILL, dtype=dt, device=cuda) for k, dt in K.PLAY_PLAN_OUTPUTS.items()}
    K.play_plan(board, hand, plan, combo, out={k: bufs[k][8:8 + n] for k in wanted})
    full = K.play_plan(board, hand, plan, combo)
    for k, v in bufs.items():
        assert (v[:8] == FILL).all() and (v[8 + n:] == FILL).all(), k
        if k in wanted:
            assert torch.equal(v[8:8 + n], full[k]), k
        else:
            assert (v == FILL).all(), f"{k} was not asked for"
    PP.check(c, full)


def test_tensors_on_the_wrong_side_are_refused(cuda):
    from runtime import kernels as K
    from runtime import lib as L

    c = PP.cases()
    board, hand, combo, plan = PP.tensors(c, "cpu")
    with pytest.raises(L.BBNativeError, match="plan must be a contiguous"):
        K.play_plan(board.to(cuda), hand.to(cuda), plan)
    with pytest.raises(L.BBNativeError, match="hand must be a contiguous"):
        K.play_plan(board.to(cuda), hand, plan.to(cuda))
    with pytest.raises(L.BBNativeError, match="status must be a contiguous"):
        K.play_plan(board, hand, plan, out={"status": torch.zeros(len(board), dtype=torch.int32, device=cuda)})
