"""Shared by tests/test_plan_values_host.py and tests/test_gpu_plan_values.py: a reference for the per-action
full-hand values (bb_plan_values) that calls none of its entry points.

Every position is expanded once with the one-ply call (``_plan_ref._expand``, the host backend's bb_afterstates,
held to the oracle by tests/test_afterstates_host.py).  A first move that ends its sequence (depth 1, refill or
dead) is a leaf of its own: q = its move terms + state terms, rest = 0xFFFF, one leaf, safe iff not dead.  Under
any other first move the child position (board', the hand with the slot marked used, combo') is searched by
``_plan_ref.chained`` at depth - 1: q = the move terms + the child's value, rest = the child's plan[:2], leaves =
the child's leaves.  The child is also searched under the weights {"dead": -1}: its best value is 0 iff some
maximal sequence ends in an afterstate that is not dead, which is "safe".
"""
import functools

import numpy as np

import _afterstates_ref as R
import _plan_ref as P

INT64_MIN = R.INT64_MIN
ALIVE = "_alive"  # the weight set that sees nothing but dead
STATE_TERMS = ("holes", "filled", "centre", "mobility", "dead", "refill")


def per_action(board, hand, combo, depth):
    """{"q": {weight set: i64 [n, 192]}, "rest": {weight set: i32 [n, 192]}, "leaves": i32 [n, 192], "safe": bool
    [n, 192], "legal", "dead1" (legal and dead on the spot): bool [n, 192]} for the positions (numpy u64 / u32 / i32
    [n]) under P.WEIGHT_SETS."""
    board, hand, combo = np.asarray(board, np.uint64), np.asarray(hand, np.uint32), np.asarray(combo, np.int64)
    n = len(board)
    q = {k: np.full((n, 192), INT64_MIN, np.int64) for k in P.WEIGHT_SETS}
    rest = {k: np.full((n, 192), -1, np.int32) for k in P.WEIGHT_SETS}
    leaves = np.zeros((n, 192), np.int32)
    safe = np.zeros((n, 192), bool)
    legal = np.zeros((n, 192), bool)
    dead1 = np.zeros((n, 192), bool)
    node, act, f = P._expand(board, hand, combo)
    legal[node, act] = True
    dead1[node, act] = f["dead"] == 1
    end = (f["refill"] == 1) | (f["dead"] == 1) | (depth == 1)
    move = {k: int(w.get("lines", 0)) * f["lines"] + int(w.get("score", 0)) * f["score"]
            for k, w in P.WEIGHT_SETS.items()}
    e = np.nonzero(end)[0]
    for k, w in P.WEIGHT_SETS.items():
        q[k][node[e], act[e]] = move[k][e] + sum(int(w.get(t, 0)) * f[t][e] for t in STATE_TERMS)
        rest[k][node[e], act[e]] = 0xFFFF
    leaves[node[e], act[e]] = 1
    safe[node[e], act[e]] = f["dead"][e] == 0
    g = np.nonzero(~end)[0]
    if g.size:
        child_hand = hand[node[g]] | (np.uint32(1) << (18 + (act[g] >> 6)).astype(np.uint32))
        child_combo = np.where(f["lines"][g] > 0, combo[node[g]] + 1, 0)
        child = P.chained(f["board"][g], child_hand, child_combo, depth - 1, {**P.WEIGHT_SETS, ALIVE: {"dead": -1}})
        for k in P.WEIGHT_SETS:
            q[k][node[g], act[g]] = move[k][g] + child[k]["value"]
            a23 = child[k]["plan"][:, :2].astype(np.int64) & 0xFF  # -1 -> 0xFF
            rest[k][node[g], act[g]] = (a23[:, 0] | (a23[:, 1] << 8)).astype(np.int32)
        leaves[node[g], act[g]] = child["default"]["leaves"]
        safe[node[g], act[g]] = child[ALIVE]["value"] == 0
    return {"q": q, "rest": rest, "leaves": leaves, "safe": safe, "legal": legal, "dead1": dead1}


@functools.lru_cache(maxsize=None)
def reference_values(depth):
    """``per_action`` on the position set of tests/_afterstates_ref.py, computed once per depth."""
    ref = R.reference()
    return per_action(ref["board"], ref["hand"], ref["combo"], depth)


def safe_bool(words):
    """Mask words [n, 3] (any 64-bit integer dtype) -> bool [n, 192], bit c of word p = action p*64 + c."""
    w = np.ascontiguousarray(words).view(np.uint64).reshape(-1, 3)
    return ((w[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1, 192)


def check(got, want, wname, idx=None, what=""):
    """All four outputs of a plan_values call (torch tensors, any device) against ``per_action``'s result."""
    sel = slice(None) if idx is None else np.asarray(idx)
    pairs = (("q", got["q"].cpu().numpy(), want["q"][wname][sel]),
             ("rest", got["rest"].cpu().numpy(), want["rest"][wname][sel]),
             ("leaves", got["leaves"].cpu().numpy(), want["leaves"][sel]),
             ("safe", safe_bool(got["safe"].cpu().numpy()), want["safe"][sel]))
    for k, g, x in pairs:
        bad = np.argwhere(g != x)[:4]
        assert bad.size == 0, (what, wname, k, bad.tolist(), [g[tuple(b)].item() for b in bad],
                               [x[tuple(b)].item() for b in bad])
