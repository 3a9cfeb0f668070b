"""Shared by tests/test_plan_host.py and tests/test_gpu_plan.py: two references for the full-hand lookahead
(bb_plan_actions) that call none of its entry points.

* ``chained``: ``search(P, d)`` of include/bbvec.h written with the one-ply call on CPU tensors
  (``runtime.kernels.afterstates``, the host backend's, held to the oracle by tests/test_afterstates_host.py) and
  numpy.  It expands level by level in batches, carries the sums of lines and score_gained and the combo, scores
  every maximal sequence and keeps per position the largest value and, among those, the lowest key
  a1 << 16 | a2 << 8 | a3 (0xFF for a ply not played), which is the lexicographic order of the sequences because
  none is a prefix of another.  It counts the maximal sequences.
* ``oracle_search``: the same search as a direct recursion on ``oracle.bb_game.Env`` with
  ``copy.deepcopy(env).step(a)``, the chance part of a refill move removed as tests/_afterstates_ref.py does.
  Slow, so for small trees only.
"""
import copy
import functools

import numpy as np
import torch

import _afterstates_ref as R
from oracle import bb_game as O

INT64_MIN = R.INT64_MIN
NO_KEY = 0xFFFFFFFF
BATCH = 16384  # nodes per one-ply call: 16,384 x 192 x 16 bytes of outputs
MIXED = {"lines": -7, "score": 3, "holes": -1, "filled": 1, "centre": 5, "mobility": -2, "dead": 50, "refill": 11}
WEIGHT_SETS = {"default": R.DEFAULT_WEIGHTS, "zero": {}, "mixed": MIXED}


def _expand(board, hand, combo):
    """The legal afterstates of the nodes (u64 / u32 / i32 arrays): node index, action and features, flat."""
    from runtime import kernels as K

    out = K.afterstates(torch.from_numpy(board.view(np.int64).copy()), torch.from_numpy(hand.view(np.int32).copy()),
                        torch.from_numpy(combo.astype(np.int32)),
                        out=K.afterstate_outputs(len(board), torch.device("cpu"), want=("board", "score_gained", "aux")))
    aux = K.unpack_aux(out["aux"].numpy())
    node, act = np.nonzero(aux["legal"])
    f = {k: aux[k][node, act].astype(np.int64) for k in ("dead", "refill", "lines", "holes", "centre", "mobility")}
    f["board"] = out["board"].numpy().view(np.uint64)[node, act]
    f["score"] = out["score_gained"].numpy()[node, act].astype(np.int64)
    f["filled"] = np.bitwise_count(f["board"]).astype(np.int64)
    return node, act.astype(np.int64), f


class _Best:
    """Per position and weight set: the best value, the lowest key among the best, the number of leaves."""

    def __init__(self, n, weight_sets):
        self.ws = weight_sets
        self.value = {k: np.full(n, INT64_MIN, np.int64) for k in weight_sets}
        self.key = {k: np.full(n, NO_KEY, np.int64) for k in weight_sets}
        self.leaves = np.zeros(n, np.int64)
        self.n = n

    def add(self, root, key, sum_lines, sum_score, f):
        if len(root) == 0:
            return
        self.leaves += np.bincount(root, minlength=self.n)
        for name, w in self.ws.items():
            v = int(w.get("lines", 0)) * sum_lines + int(w.get("score", 0)) * sum_score
            for k in ("holes", "filled", "centre", "mobility", "dead", "refill"):
                v = v + int(w.get(k, 0)) * f[k]
            top = np.full(self.n, INT64_MIN, np.int64)
            np.maximum.at(top, root, v)
            better = top > self.value[name]
            self.value[name][better] = top[better]
            self.key[name][better] = NO_KEY
            tie = v == self.value[name][root]
            np.minimum.at(self.key[name], root[tie], key[tie])


def chained(board, hand, combo, depth, weight_sets=None):
    """search(P, depth) for the positions (numpy u64 / u32 / i32 [n]) under every weight set of the dict
    ``weight_sets`` (default WEIGHT_SETS).  Returns {name: {"action", "value", "plan" [n, 3], "leaves"}} plus, under
    "_stats", what the best plans and the trees look like (for the tests' non-vacuity assertions)."""
    weight_sets = WEIGHT_SETS if weight_sets is None else weight_sets
    n = len(board)
    best = _Best(n, weight_sets)
    dead_before_depth = np.zeros(n, bool)
    # a level's nodes: root, board, hand, combo, key so far, sums so far
    level = [(np.arange(n), np.asarray(board, np.uint64), np.asarray(hand, np.uint32), np.asarray(combo, np.int64),
              np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64))]
    for ply in range(1, depth + 1):
        nxt = []
        shift = 8 * (3 - ply)
        absent = (1 << shift) - 1  # 0xFF in every ply below this one
        for root, b, h, c, key, sl, ss in level:
            for lo in range(0, len(root), BATCH):
                s = slice(lo, lo + BATCH)
                node, act, f = _expand(b[s], h[s], c[s])
                r = root[s][node]
                k = key[s][node] | (act << shift)
                lines, score = sl[s][node] + f["lines"], ss[s][node] + f["score"]
                end = (f["refill"] == 1) | (f["dead"] == 1) | (ply == depth)
                best.add(r[end], k[end] | absent, lines[end], score[end], {x: y[end] for x, y in f.items()})
                if ply < depth:
                    dead_before_depth[r[f["dead"] == 1]] = True
                go = ~end
                if go.any():
                    nxt.append((r[go], f["board"][go], h[s][node][go] | (np.uint32(1) << (18 + (act[go] >> 6)).astype(np.uint32)),
                                np.where(f["lines"][go] > 0, c[s][node][go] + 1, 0), k[go], lines[go], score[go]))
        level = nxt
    res = {}
    for name in weight_sets:
        key, found = best.key[name], best.key[name] != NO_KEY
        plan = np.stack([(key >> 16) & 0xFF, (key >> 8) & 0xFF, key & 0xFF], axis=1)
        plan = np.where((plan == 0xFF) | ~found[:, None], -1, plan).astype(np.int32)
        res[name] = {"action": np.where(found, plan[:, 0], 0).astype(np.int32), "value": best.value[name],
                     "plan": plan, "leaves": best.leaves.astype(np.int32)}
    res["_stats"] = {"dead_before_depth": dead_before_depth}
    return res


@functools.lru_cache(maxsize=None)
def reference_plans(depth):
    """``chained`` on the position set of tests/_afterstates_ref.py under WEIGHT_SETS, computed once per depth."""
    ref = R.reference()
    return chained(ref["board"], ref["hand"], ref["combo"], depth)


def plan_lines(board, hand, combo, plan):
    """Lines cleared and score gained by each move of one position's plan (a list of up to three actions, -1
    ends it), by playing it through the one-ply call."""
    b, h, c = np.array([board], np.uint64), np.array([hand], np.uint32), np.array([combo], np.int64)
    lines, gained = [], []
    for a in plan:
        if a < 0:
            break
        node, act, f = _expand(b, h, c)
        j = int(np.nonzero(act == a)[0][0])
        lines.append(int(f["lines"][j]))
        gained.append(int(f["score"][j]))
        b, h = f["board"][j:j + 1], h | (np.uint32(1) << np.uint32(18 + (a >> 6)))
        c = np.array([c[0] + 1 if lines[-1] > 0 else 0], np.int64)
    return lines, gained


def oracle_search(env, depth, weights):
    """(value, plan, leaves) of search(P, depth) by recursion on copies of the oracle env."""
    best = {"value": INT64_MIN, "plan": [-1, -1, -1], "leaves": 0}

    def rec(env, d, total, seq):
        for a in range(192):  # ascending at every ply: lexicographic order, a later leaf must be strictly better
            p, r, c = O.Env.action_to_move(a)
            if not env.engine.can_place_piece(p, r, c):
                continue
            refill = sum(env.engine.used) == 2
            cp = copy.deepcopy(env)
            if refill:  # the new hand and whether it fits are chance: left out
                cp.engine._generate = lambda: None
                cp.engine.has_valid_moves = lambda: True
            _, _, term, _, info = cp.step(a)
            lm = info["last_move"]
            s = total + int(weights.get("lines", 0)) * lm["lines_cleared"] + int(weights.get("score", 0)) * lm["score_gained"]
            if d == 1 or refill or term:
                g = cp.engine.grid
                res = {"holes": O.count_holes(g), "centre": O.center_filled(g), "filled": O.total_blocks(g),
                       "mobility": len(cp.engine.valid_moves()), "dead": int(term), "refill": int(refill)}
                v = s + sum(int(weights.get(k, 0)) * res[k] for k in res)
                best["leaves"] += 1
                if best["leaves"] == 1 or v > best["value"]:
                    best["value"], best["plan"] = v, (seq + [a] + [-1, -1])[:3]
            else:
                rec(cp, d - 1, s, seq + [a])

    rec(env, depth, 0, [])
    return best["value"], best["plan"], best["leaves"]


def unused_slots(hand):
    """Number of unused hand slots per packed hand word."""
    return 3 - np.bitwise_count((np.asarray(hand, np.uint32) >> 18) & 7)
