"""The rules atlas through every HIP kernel that contains the move, against the unmodified oracle.

The oracle comparisons of the env kernels otherwise run on positions that play produces: at most 3-4 lines per move
and a combo of about 5, so apply_move (step_kernel), apply_move_bf (the fused step) and rollout_async_kernel (the
kernel the bench times) never meet a capped streak min(combo + 1, 8), a 5- or 6-line clear, or a max_combo update
from a high combo, and the tuned device geometry (the byte-permute clear_full, the Minkowski anchors_of program, the
LDS piece table) is checked only where play happens to hit it.  tests/_rules_atlas.py builds those positions --
every piece at every anchor, 0 to 6 lines, combos on both sides of the cap, refill and game-ending moves, blocker
boards -- and the oracle's answer; one case per kernel compares every output, the info record and the whole
post-move state.  Every comparison is exact (integers and fp64 rewards with ==, fp32 rewards by their bits); a
failure names the position (piece, anchor, variant, combo) and the differing field.
tests/test_rules_atlas_host.py runs the same comparisons on the host backend.
"""
import numpy as np
import pytest

import _rules_atlas as A

pytestmark = pytest.mark.gpu

STEP_KERNELS = {"fused": "1", "step+escalate": "2"}  # apply_move_bf at T = 1; step_kernel + escalate_kernel


@pytest.mark.parametrize("kernels", list(STEP_KERNELS))
def test_step_matches_oracle_on_every_position(cuda, kernels, monkeypatch):
    monkeypatch.setenv("BB_STEP_KERNELS", STEP_KERNELS[kernels])
    print(A.summary(A.reference()))
    A.check_step(cuda)


@pytest.mark.parametrize("kernels", list(STEP_KERNELS))
def test_step_matches_oracle_under_custom_rewards(cuda, kernels, monkeypatch):
    monkeypatch.setenv("BB_STEP_KERNELS", STEP_KERNELS[kernels])
    A.check_step(cuda, custom=True)


def test_rollout_matches_oracle_replay(cuda):
    """rollout_async_kernel (T = 3, auto-reset), the crafted action first."""
    A.check_rollout(cuda)


def test_afterstates_pos_match_oracle(cuda):
    from runtime import kernels as K

    A.check_afterstates(K.afterstates(*A.position_tensors(A.positions(), cuda)))


@pytest.mark.parametrize("idx", [[0], list(range(67))], ids=["n=1", "n=67"])
def test_afterstates_pos_small_and_ragged(cuda, idx):
    from runtime import kernels as K

    A.check_afterstates(K.afterstates(*A.position_tensors(A.positions(), cuda, np.array(idx))), idx)


def test_afterstates_handle_form_matches_oracle(cuda):
    batch = A.make_batch(cuda, autoreset=False)
    out = batch.afterstates()
    batch.sync()
    A.check_afterstates(out)
    batch.close()


@pytest.mark.parametrize("part", [None, [0], list(range(67))], ids=["subset", "n=1", "n=67"])
def test_greedy_and_plan_on_one_piece_left(cuda, part):
    A.check_greedy_and_plan(cuda, part)


def test_blocker_boards(cuda):
    A.check_blockers(cuda)
