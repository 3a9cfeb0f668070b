"""Shared by tests/test_play_plan_host.py and tests/test_gpu_play_plan.py: positions, plans of 0-3 plies and what the
oracle env makes of them.  Nothing here calls bb_play_plan_pos.

The positions are those of tests/_afterstates_ref.py (played games and crafted boards).  Every position gets its best
full-hand plan (the host backend's bb_plan_actions, held to its references by tests/test_plan_host.py), that plan cut
to one and two plies, no plan at all, a single move that leaves the hand dead where the position has one, the plan
with its second ply replaced by the first (the slot is used by then: illegal), and an entry past the 192 actions.
"""
import copy
import functools

import numpy as np
import torch

import _afterstates_ref as R
from oracle import bb_game as O

PLIES, DEAD, REFILL, ILLEGAL = 3, 4, 8, 16


def oracle_play(env, plan):
    """(board, used bits, combo, lines, score, status) of the plan played on a copy of the oracle env, the chance part
    of a refill move left out as tests/_afterstates_ref.py leaves it out."""
    cp = copy.deepcopy(env)
    lines = score = status = 0
    used = sum(int(u) << s for s, u in enumerate(cp.engine.used))
    for k, a in enumerate(plan):
        if a < 0:
            break
        if a >= 192 or not cp.engine.can_place_piece(*O.Env.action_to_move(a)):
            status |= ILLEGAL
            break
        refill = sum(cp.engine.used) == 2
        if refill:
            cp.engine._generate = lambda: None
            cp.engine.has_valid_moves = lambda: True
        _, _, term, _, info = cp.step(a)
        lines += info["last_move"]["lines_cleared"]
        score += info["last_move"]["score_gained"]
        used |= 1 << (a >> 6)
        status = (k + 1) | (DEAD if term else 0) | (REFILL if refill else 0)
    return O.grid_to_u64(cp.engine.grid), used, cp.engine.combo, lines, score, status


@functools.lru_cache(maxsize=None)
def cases():
    """{"board", "hand", "combo", "plan" [n, 3], "env" (index of the oracle env)} and the expectation {"exp_board",
    "exp_hand", "exp_combo", "exp_lines", "exp_score", "exp_status"}; the three status bits are asserted to occur."""
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    ref = R.reference()
    board, hand, combo = R.tensors(ref, "cpu")[:3]
    best = K.plan_actions(board, hand, P_WEIGHTS, 3, combo=combo, want_plan=True)["plan"].numpy()
    rows = []
    for i in range(ref["n"]):
        p = best[i].tolist()
        plans = [p, [p[0], -1, -1], [p[0], p[1], -1], [-1, -1, -1], [p[0], p[0], p[2]], [192, p[1], -1],
                 [p[0], 255, -1], [-1, p[0], p[1]]]
        dead = np.nonzero(ref["dead"][i] == 1)[0]
        if len(dead):
            plans.append([int(dead[0]), -1, -1])
            plans.append([int(dead[-1]), p[0], -1])  # nothing fits after a dead move: the second ply is illegal
        rows += [(i, q) for q in plans]
    idx = np.array([i for i, _ in rows])
    out = {"env": idx, "board": ref["board"][idx], "hand": ref["hand"][idx], "combo": ref["combo"][idx],
           "plan": np.array([q for _, q in rows], np.int32)}
    exp = [oracle_play(ref["envs"][i], q) for i, q in rows]
    out["exp_board"] = np.array([e[0] for e in exp], np.uint64)
    out["exp_hand"] = (out["hand"] | np.array([e[1] << 18 for e in exp], np.uint32)).astype(np.uint32)
    for col, k in enumerate(("exp_combo", "exp_lines", "exp_score", "exp_status"), start=2):
        out[k] = np.array([e[col] for e in exp], np.int64)
    st = out["exp_status"]
    for plies in range(4):
        assert ((st & PLIES) == plies).sum() >= 3, plies
    assert ((st & DEAD) != 0).sum() >= 2 and ((st & REFILL) != 0).sum() >= 3 and ((st & ILLEGAL) != 0).sum() >= 3
    assert (((st & ILLEGAL) != 0) & ((st & PLIES) > 0)).any() and (out["exp_lines"] > 0).any()
    for v in out.values():
        v.setflags(write=False)
    return out


P_WEIGHTS = R.DEFAULT_WEIGHTS


def tensors(c, dev):
    """board i64, hand i32, combo i32, plan i32 [n, 3] of the cases on ``dev``."""
    return (torch.from_numpy(c["board"].view(np.int64).copy()).to(dev),
            torch.from_numpy(c["hand"].view(np.int32).copy()).to(dev),
            torch.from_numpy(c["combo"].astype(np.int32)).to(dev), torch.from_numpy(c["plan"].copy()).to(dev))


def check(c, got):
    """The outputs of play_plan (a dict of tensors) against the expectation."""
    assert got["board"].cpu().numpy().view(np.uint64).tolist() == c["exp_board"].tolist()
    assert got["hand"].cpu().numpy().view(np.uint32).tolist() == c["exp_hand"].tolist()
    for k in ("combo", "lines", "score", "status"):
        assert got[k].cpu().tolist() == c["exp_" + k].tolist(), k
