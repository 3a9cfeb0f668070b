"""Shared by the tests of bb_plan_values_ext / bb_refill_values_ext (tests/test_values_ext_host.py,
tests/test_gpu_values_ext.py, tests/test_two_hand_shape_host.py): references that call none of the new entry points,
composed from the references the parents' tests already use.

* ``per_action_ext``: tests/_plan_values_ref.py's ``per_action`` under the twelve-weight sets of
  tests/_eval_terms_ref.py.  A first move that ends its sequence adds ``cell_terms`` of its own board to its value;
  below any other first move the child position is searched by ``chained_ext`` at depth - 1, which adds the terms of
  every leaf's board.  ``safe`` comes from the child searched under {"dead": -1}, as there.
* ``refill_values_ext``: tests/_refill_values_ref.py's ``deal`` for the hands and the attempts, then ``chained_ext``
  on (board, hand, combo); a hand with no legal first move is priced at the set's ``dead``.  Boards that one move
  can empty go through a recursion on the oracle env instead (``chained_ext`` reads a move's lines from an aux word
  with four bits, as ``_refill_values_ref.search`` explains), with ``cell_terms`` of the leaf's grid added.

``reference_values`` asserts its own non-vacuity from its own answers: per position max_a q, its lowest arg-max, the
decoded rest and the sum of leaves equal ``chained_ext``'s value, action, plan and leaves, and on the whole set at
depth 3 the pair (arg-max action, rest[arg-max]) differs from zero4's at >= 5 positions under every single-term set
and at >= 40 under ``all``.
"""
import copy
import functools

import numpy as np

import _afterstates_ref as R
import _eval_terms_ref as E
import _plan_ref as P
import _plan_values_ref as V
import _refill_values_ref as RV

INT64_MIN = R.INT64_MIN
SETS = E.SETS
NAMES = list(SETS)
ALIVE = V.ALIVE


def _terms_value(w, t):
    return sum(int(w.get(k, 0)) * t[:, j] for j, k in enumerate(E.TERMS))


def per_action_ext(board, hand, combo, depth, weight_sets=None):
    """``_plan_values_ref.per_action`` under weight sets that may name the shape terms: {"q": {set: i64 [n, 192]},
    "rest": {set: i32 [n, 192]}, "leaves" i32 [n, 192], "safe" bool [n, 192], "legal" bool [n, 192]}."""
    ws = SETS if weight_sets is None else weight_sets
    board, hand, combo = np.asarray(board, np.uint64), np.asarray(hand, np.uint32), np.asarray(combo, np.int64)
    n = len(board)
    q = {k: np.full((n, 192), INT64_MIN, np.int64) for k in ws}
    rest = {k: np.full((n, 192), -1, np.int32) for k in ws}
    leaves = np.zeros((n, 192), np.int32)
    safe = np.zeros((n, 192), bool)
    legal = np.zeros((n, 192), bool)
    node, act, f = P._expand(board, hand, combo)
    legal[node, act] = True
    end = (f["refill"] == 1) | (f["dead"] == 1) | (depth == 1)
    move = {k: int(w.get("lines", 0)) * f["lines"] + int(w.get("score", 0)) * f["score"] for k, w in ws.items()}
    e = np.nonzero(end)[0]
    if e.size:
        t = E.cell_terms(f["board"][e])
        for k, w in ws.items():
            q[k][node[e], act[e]] = (move[k][e] + sum(int(w.get(s, 0)) * f[s][e] for s in V.STATE_TERMS)
                                     + _terms_value(w, t))
            rest[k][node[e], act[e]] = 0xFFFF
        leaves[node[e], act[e]] = 1
        safe[node[e], act[e]] = f["dead"][e] == 0
    g = np.nonzero(~end)[0]
    if g.size:
        child_hand = hand[node[g]] | (np.uint32(1) << (18 + (act[g] >> 6)).astype(np.uint32))
        child_combo = np.where(f["lines"][g] > 0, combo[node[g]] + 1, 0)
        child = E.chained_ext(f["board"][g], child_hand, child_combo, depth - 1, {**ws, ALIVE: {"dead": -1}})
        for k in ws:
            q[k][node[g], act[g]] = move[k][g] + child[k]["value"]
            a23 = child[k]["plan"][:, :2].astype(np.int64) & 0xFF  # -1 -> 0xFF
            rest[k][node[g], act[g]] = (a23[:, 0] | (a23[:, 1] << 8)).astype(np.int32)
        leaves[node[g], act[g]] = child[ALIVE]["leaves"]
        safe[node[g], act[g]] = child[ALIVE]["value"] == 0
    return {"q": q, "rest": rest, "leaves": leaves, "safe": safe, "legal": legal}


def best_pair(res, name):
    """(arg-max action, rest[arg-max]) per position under set ``name``; (0, -1) without a legal action."""
    q = res["q"][name]
    a = q.argmax(axis=1)  # the lowest arg-max
    return a, res["rest"][name][np.arange(len(a)), a]


def pairs_changed(res, name):
    a, r = best_pair(res, name)
    a0, r0 = best_pair(res, "zero4")
    return int(((a != a0) | (r != r0)).sum())


@functools.lru_cache(maxsize=None)
def reference_values(depth, whole=True):
    """``per_action_ext`` on the position set of tests/_afterstates_ref.py under SETS, once per (depth, whole);
    whole=False: the small depth-3 trees (``_eval_terms_ref.small_index``).  Returns (index, result).  Held to
    ``chained_ext`` position by position, and non-vacuous by the counts of the module docstring."""
    ref = R.reference()
    idx, plans = E.reference_plans(depth, whole)
    res = per_action_ext(ref["board"][idx], ref["hand"][idx], ref["combo"][idx], depth)
    for name in SETS:
        a, r = best_pair(res, name)
        want, found = plans[name], plans[name]["leaves"] > 0
        assert np.array_equal(res["q"][name].max(axis=1), want["value"]), name
        assert np.array_equal(np.where(found, a, 0), want["action"]), name
        a23 = want["plan"][:, 1:].astype(np.int64) & 0xFF
        assert np.array_equal(r[found], (a23[:, 0] | (a23[:, 1] << 8))[found]), name
        assert np.array_equal(res["leaves"].sum(axis=1), want["leaves"]), name
    if whole and depth == 3:
        changed = {k: pairs_changed(res, k) for k in SETS if k != "zero4"}
        assert all(changed[k] >= 5 for k in E.SINGLE_TERM_SETS), changed
        assert changed["all"] >= 40, changed
    for v in (*res["q"].values(), *res["rest"].values(), res["leaves"], res["safe"], res["legal"]):
        v.setflags(write=False)
    return idx, res


def check(got, want, name, sel=None, what=""):
    """All four outputs of a plan_values_ext call (torch tensors, any device; missing ones skipped) against
    ``per_action_ext``'s result under set ``name``."""
    sel = slice(None) if sel is None else np.asarray(sel)
    pairs = [("q", lambda g: g, want["q"][name][sel]), ("rest", lambda g: g, want["rest"][name][sel]),
             ("leaves", lambda g: g, want["leaves"][sel]), ("safe", V.safe_bool, want["safe"][sel])]
    for k, conv, x in pairs:
        if got.get(k) is None:
            continue
        g = conv(got[k].cpu().numpy())
        bad = np.argwhere(g != x)[:4]
        assert bad.size == 0, (what, name, k, bad.tolist(), [g[tuple(b)].item() for b in bad],
                               [x[tuple(b)].item() for b in bad])


# ---------------------------------------------------------------------------------------------------------------
# dealt next-hand values
# ---------------------------------------------------------------------------------------------------------------
def _oracle_leaves(env, depth):
    """The maximal sequences of search(P, depth) on the oracle env, ``_plan_ref.oracle_search``'s recursion with the
    leaves kept: a list of (sum of lines, sum of score gained, features of the last afterstate, its board bits)."""
    O = P.O
    out = []

    def rec(env, d, lines, score):
        for a in range(192):
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
            sl, ss = lines + lm["lines_cleared"], score + lm["score_gained"]
            if d == 1 or refill or term:
                g = cp.engine.grid
                bits = sum(1 << (rr * 8 + cc) for rr in range(8) for cc in range(8) if g[rr][cc])
                out.append((sl, ss, {"holes": O.count_holes(g), "centre": O.center_filled(g),
                                     "filled": O.total_blocks(g), "mobility": len(cp.engine.valid_moves()),
                                     "dead": int(term), "refill": int(refill)}, bits))
            else:
                rec(cp, d - 1, sl, ss)

    rec(env, depth, 0, 0)
    return out


def _oracle_values(board, hand, combo, depth, ws):
    """{set: best value or None without a leaf} of one position whole-hand on the oracle env."""
    lv = _oracle_leaves(RV._oracle_env(board, hand, combo), depth)
    if not lv:
        return {k: None for k in ws}
    t = E.cell_terms(np.array([x[3] for x in lv], np.uint64))
    res = {}
    for k, w in ws.items():
        v = np.array([int(w.get("lines", 0)) * sl + int(w.get("score", 0)) * ss + sum(int(w.get(s, 0)) * f[s] for s in f)
                      for sl, ss, f, _ in lv], np.int64) + _terms_value(w, t)
        res[k] = int(v.max())
    return res


def refill_values_ext(boards, deals, seed, depth, weight_sets=None, combo=None, stream=None):
    """{"hand" u32 [n, deals], "attempts" i32 [n, deals], "value": {set: i64 [n, deals]}, "leaves" [n, deals]}: the
    whole call restated under every weight set (each set prices every board: a per-board choice is the caller's)."""
    ws = SETS if weight_sets is None else weight_sets
    boards = np.asarray(boards, np.uint64)
    hand, attempts = RV.deal(boards, deals, seed, stream)
    n, m = hand.shape
    combo = np.zeros(n, np.int32) if combo is None else np.asarray(combo, np.int32)
    value = {k: np.zeros((n, m), np.int64) for k in ws}
    leaves = np.zeros((n, m), np.int64)
    open_ = np.array([bin(int(b)).count("1") < RV.CROWDED_CELLS for b in boards])
    if open_.any():
        res = E.chained_ext(np.repeat(boards[open_], m), hand[open_].reshape(-1).astype(np.uint32),
                            np.repeat(combo[open_], m), depth, ws)
        for k, w in ws.items():
            lv = res[k]["leaves"].reshape(-1, m)
            value[k][open_] = np.where(lv == 0, np.int64(w.get("dead", 0)), res[k]["value"].reshape(-1, m))
            leaves[open_] = lv
    for i in np.nonzero(~open_)[0]:
        for j in range(m):
            got = _oracle_values(boards[i], hand[i, j], combo[i], depth, ws)
            for k, w in ws.items():
                value[k][i, j] = int(w.get("dead", 0)) if got[k] is None else got[k]
            leaves[i, j] = 0 if got[next(iter(ws))] is None else 1  # some leaf or none: all the tests ask
    return {"hand": hand, "attempts": attempts, "value": value, "leaves": leaves}


@functools.lru_cache(maxsize=None)
def refill_boards():
    """(boards u64, combo i32, stream i64) of the refill tests: ``_refill_values_ref.FIXED_BOARDS`` plus mid-game
    boards of the position set with their combos; stream ids shared in pairs, so two boards meet the same draws."""
    ref = R.reference()
    filled = np.array([bin(int(b)).count("1") for b in ref["board"]])
    mid = np.nonzero((filled >= 24) & (filled < RV.CROWDED_CELLS))[0]  # the depth-3 trees of a dealt hand stay small
    pick = mid[np.linspace(0, len(mid) - 1, 6).astype(int)]
    assert len(set(pick.tolist())) == 6
    boards = np.concatenate([RV.FIXED_BOARDS, ref["board"][pick]])
    combo = np.concatenate([np.zeros(len(RV.FIXED_BOARDS), np.int32), ref["combo"][pick].astype(np.int32)])
    stream = (np.arange(len(boards)) // 2 + 5).astype(np.int64)
    return boards, combo, stream


REFILL_SEED = 7
REFILL_CASES = ((1, 3), (3, 2), (16, 1))  # (deals, depth): the trees of 16 deals at depth 3 are the GPU's to search


@functools.lru_cache(maxsize=None)
def reference_refill(deals, depth):
    boards, combo, stream = refill_boards()
    res = refill_values_ext(boards, deals, REFILL_SEED, depth, combo=combo, stream=stream)
    if deals >= 3:  # what the boards are for: accepted late, refused, and no legal first move at all
        at = res["attempts"]
        assert (at == 1).any() and ((at > 1) & (at < RV.ATTEMPTS)).any() and (at == -RV.ATTEMPTS).any()
        assert (res["leaves"] == 0).any() and (res["leaves"] > 0).any()
        assert (res["value"]["all"] != res["value"]["zero4"]).any()
    return res
