"""The rules atlas through the host backend (libbbvec_host.so, csrc/bb_host.cpp), on the CPU (no GPU involved).

csrc/bb_rules.h is compiled into both the HIP kernels and the host backend, so a wrong rule is wrong on both sides
at once and only the oracle can tell.  tests/_rules_atlas.py builds positions that play does not reach -- every
piece at every anchor, clears of 0 to 6 lines, combos on both sides of the streak cap, refill moves, game-ending
moves, blocker boards -- and the oracle's answer for each; here every entry point of the host backend that contains
the move is compared with it.  Every comparison is exact (integers and fp64 rewards with ==, fp32 rewards by their
bits); a failure names the position (piece, anchor, variant, combo) and the differing field.
"""
import numpy as np
import pytest
import torch

import _rules_atlas as A

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


def test_atlas_covers_what_play_does_not():
    """The coverage conditions hold on the oracle alone (asserted while the reference is built); the counts."""
    ref = A.reference()
    print(A.summary(ref))
    assert ref["n"] == 5 * len(A.pairs()) <= 8500
    assert ref["capped"].sum() >= 1000 and ref["term"].sum() >= 100
    assert ref["chance_end"].sum() * 100 <= ref["n"]
    blk = A.blockers()
    assert blk["n"] == 64 * 13 + len(A.pairs())


def test_step_matches_oracle_on_every_position(host):
    A.check_step(CPU)


def test_step_matches_oracle_under_custom_rewards(host):
    A.check_step(CPU, custom=True)
    # the custom config changes the reward of (nearly) every move: the second pass is not the first again
    assert (A.reference(True)["reward"] != A.reference()["reward"]).mean() > 0.9


def test_rollout_matches_oracle_replay(host):
    A.check_rollout(CPU)


def test_afterstates_pos_match_oracle(host):
    from runtime import kernels as K

    A.check_afterstates(K.afterstates(*A.position_tensors(A.positions(), CPU)))


@pytest.mark.parametrize("idx", [[0], list(range(67))], ids=["n=1", "n=67"])
def test_afterstates_pos_small_and_ragged(host, idx):
    from runtime import kernels as K

    A.check_afterstates(K.afterstates(*A.position_tensors(A.positions(), CPU, np.array(idx))), idx)


def test_afterstates_handle_form_matches_oracle(host):
    batch = A.make_batch(CPU, autoreset=False)
    A.check_afterstates(batch.afterstates())
    batch.close()


def test_greedy_and_plan_on_one_piece_left(host):
    assert 250 <= len(A.greedy_subset()) <= 350
    A.check_greedy_and_plan(CPU)
    A.check_greedy_and_plan(CPU, [0])
    A.check_greedy_and_plan(CPU, list(range(67)))


def test_blocker_boards(host):
    A.check_blockers(CPU)
