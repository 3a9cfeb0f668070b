"""Shared by tests/test_eval_terms_host.py and tests/test_gpu_eval_terms.py: references for the shape terms
(bb_board_terms) and for the search with them (bb_plan_actions_ext) that call none of the new entry points.

* ``cell_terms``: perimeter, room3, room5 and fits restated cell by cell on an 8x8 grid of booleans.  "Fits" is
  Board.can_place: every cell of the piece (``game.pieces`` cell lists) on the board and empty, tried at every anchor.
  No shifts of whole boards, no popcounts.
* ``chained_ext``: tests/_plan_ref.py's level-by-level expansion (``_expand``, its keys and its tie handling in
  ``_Best``) with the four terms of every leaf's board added to the leaf's value.
* ``SETS``: the fixed weight sets, built on DEFAULT_WEIGHTS.

``reference_plans`` asserts its own non-vacuity, from its own answers alone: the leaves it scored include refill,
dead and depth-cut ones, and on the whole 92-position set at depth 3 every single-term set changes the best plan of
at least 5 positions against ``zero4`` and ``all`` of at least 40.
"""
import functools

import numpy as np

import _afterstates_ref as R
import _plan_ref as P

TERMS = ("perimeter", "room3", "room5", "fits")
BIG = 2 ** 31 - 1
D = dict(R.DEFAULT_WEIGHTS)
SETS = {
    "zero4": dict(D),
    "per": {**D, "perimeter": -3},
    "r3": {**D, "room3": 4},
    "r5": {**D, "room5": 2},
    "fit": {**D, "fits": 25},
    "all": {**D, "perimeter": -3, "room3": 4, "room5": 2, "fits": 25},
    # both signs, large magnitudes, one new term at the end of int32
    "mixed": {"lines": -7, "score": 3, "holes": -100003, "filled": 1, "centre": 5, "mobility": -2, "dead": 50,
              "refill": 11, "perimeter": 70001, "room3": -BIG, "room5": 900001, "fits": -12345},
}
SINGLE_TERM_SETS = ("per", "r3", "r5", "fit")
SMALL_TREE = 20000  # depth-3 trees of at most this many leaves are searched in the quick tests
_CHUNK = 8192


def _pieces():
    from game.pieces import PIECE_LIST

    return [(p.name, p.blocks) for p in PIECE_LIST]


def cell_terms(boards):
    """int64 [n, 4]: perimeter, room3, room5, fits of the boards (u64 [n], bit r*8+c = cell (r, c) filled)."""
    boards = np.asarray(boards, np.uint64).reshape(-1)
    out = np.zeros((len(boards), 4), np.int64)
    pieces = _pieces()
    for lo in range(0, len(boards), _CHUNK):
        b = boards[lo:lo + _CHUNK]
        n = len(b)
        filled = np.zeros((n, 8, 8), bool)
        for r in range(8):
            for c in range(8):
                filled[:, r, c] = (b // np.uint64(2 ** (r * 8 + c))) % np.uint64(2) == 1
        # perimeter: a frame of "filled" stands for off the board
        wall = np.ones((n, 10, 10), bool)
        wall[:, 1:9, 1:9] = filled
        per = np.zeros(n, np.int64)
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            per += (~filled & wall[:, 1 + dr:9 + dr, 1 + dc:9 + dc]).sum(axis=(1, 2))
        # fits: a margin of "not empty" stands for off the board
        empty = np.zeros((n, 13, 13), bool)
        empty[:, :8, :8] = ~filled
        fits = np.zeros(n, np.int64)
        count = {}
        for name, blocks in pieces:
            ok = np.ones((n, 8, 8), bool)  # ok[:, r, c]: the piece fits with its origin at (r, c)
            for dr, dc in blocks:
                ok &= empty[:, dr:dr + 8, dc:dc + 8]
            count[name] = ok.sum(axis=(1, 2))
            fits += count[name] > 0
        out[lo:lo + n, 0] = per
        out[lo:lo + n, 1] = count["SQUARE_3x3"]
        out[lo:lo + n, 2] = count["I5_H"] + count["I5_V"]
        out[lo:lo + n, 3] = fits
    return out


class _BestExt(P._Best):
    """``_plan_ref._Best`` with the four shape terms of the leaf's board in the value; counts the kinds of leaves."""

    def __init__(self, n, weight_sets):
        super().__init__(n, weight_sets)
        self.kinds = {"refill": 0, "dead": 0, "cut": 0}
        self.term_min = np.full(4, 10 ** 9, np.int64)
        self.term_max = np.full(4, -1, np.int64)

    def add(self, root, key, sum_lines, sum_score, f):
        if len(root) == 0:
            return
        t = cell_terms(f["board"])
        self.term_min, self.term_max = np.minimum(self.term_min, t.min(axis=0)), np.maximum(self.term_max, t.max(axis=0))
        self.kinds["refill"] += int((f["refill"] == 1).sum())
        self.kinds["dead"] += int((f["dead"] == 1).sum())
        self.kinds["cut"] += int(((f["refill"] == 0) & (f["dead"] == 0)).sum())
        self.leaves += np.bincount(root, minlength=self.n)
        for name, w in self.ws.items():
            v = int(w.get("lines", 0)) * sum_lines + int(w.get("score", 0)) * sum_score
            for k in ("holes", "filled", "centre", "mobility", "dead", "refill"):
                v = v + int(w.get(k, 0)) * f[k]
            for j, k in enumerate(TERMS):
                v = v + int(w.get(k, 0)) * t[:, j]
            top = np.full(self.n, P.INT64_MIN, np.int64)
            np.maximum.at(top, root, v)
            better = top > self.value[name]
            self.value[name][better] = top[better]
            self.key[name][better] = P.NO_KEY
            tie = v == self.value[name][root]
            np.minimum.at(self.key[name], root[tie], key[tie])


def chained_ext(board, hand, combo, depth, weight_sets=None):
    """``_plan_ref.chained`` under weight sets that may name the shape terms: {name: {"action", "value", "plan",
    "leaves"}} plus "_stats" (the kinds of leaves scored, the ranges of the terms at the leaves)."""
    weight_sets = SETS if weight_sets is None else weight_sets
    n = len(board)
    best = _BestExt(n, weight_sets)
    level = [(np.arange(n), np.asarray(board, np.uint64), np.asarray(hand, np.uint32), np.asarray(combo, np.int64),
              np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64))]
    for ply in range(1, depth + 1):
        nxt = []
        shift = 8 * (3 - ply)
        absent = (1 << shift) - 1
        for root, b, h, c, key, sl, ss in level:
            for lo in range(0, len(root), P.BATCH):
                s = slice(lo, lo + P.BATCH)
                node, act, f = P._expand(b[s], h[s], c[s])
                r = root[s][node]
                k = key[s][node] | (act << shift)
                lines, score = sl[s][node] + f["lines"], ss[s][node] + f["score"]
                end = (f["refill"] == 1) | (f["dead"] == 1) | (ply == depth)
                best.add(r[end], k[end] | absent, lines[end], score[end], {x: y[end] for x, y in f.items()})
                go = ~end
                if go.any():
                    nxt.append((r[go], f["board"][go],
                                h[s][node][go] | (np.uint32(1) << (18 + (act[go] >> 6)).astype(np.uint32)),
                                np.where(f["lines"][go] > 0, c[s][node][go] + 1, 0), k[go], lines[go], score[go]))
        level = nxt
    res = {}
    for name in weight_sets:
        key, found = best.key[name], best.key[name] != P.NO_KEY
        plan = np.stack([(key >> 16) & 0xFF, (key >> 8) & 0xFF, key & 0xFF], axis=1)
        plan = np.where((plan == 0xFF) | ~found[:, None], -1, plan).astype(np.int32)
        res[name] = {"action": np.where(found, plan[:, 0], 0).astype(np.int32), "value": best.value[name],
                     "plan": plan, "leaves": best.leaves.astype(np.int32)}
    res["_stats"] = {"kinds": dict(best.kinds), "term_min": best.term_min, "term_max": best.term_max}
    return res


def plans_changed(res, name):
    """The number of positions whose best plan under set ``name`` differs from that under zero4."""
    return int((res[name]["plan"] != res["zero4"]["plan"]).any(axis=1).sum())


@functools.lru_cache(maxsize=None)
def reference_plans(depth, whole=True):
    """``chained_ext`` on the position set of tests/_afterstates_ref.py under SETS, computed once per (depth, whole).
    whole=False: the small trees only (``small_index``), for depth 3.  Returns (index of the positions, results)."""
    ref = R.reference()
    idx = np.arange(ref["n"]) if whole else small_index()
    res = chained_ext(ref["board"][idx], ref["hand"][idx], ref["combo"][idx], depth)
    kinds = res["_stats"]["kinds"]
    assert kinds["refill"] > 0 and kinds["dead"] > 0, kinds
    assert (kinds["cut"] > 0) == (depth < 3), kinds  # at depth 3 every leaf ended its hand or died
    if whole and depth == 3:
        changed = {k: plans_changed(res, k) for k in SETS if k != "zero4"}
        assert all(changed[k] >= 5 for k in SINGLE_TERM_SETS), changed
        assert changed["all"] >= 40, changed
    return idx, res


@functools.lru_cache(maxsize=None)
def small_index():
    """The positions whose depth-3 tree has at most SMALL_TREE leaves, by the reference's own count: the leaves
    column of tests/_plan_ref.py's expansion (computed once per process, shared with the plan tests)."""
    return np.nonzero(P.reference_plans(3)["default"]["leaves"] <= SMALL_TREE)[0]


FULL = 2 ** 64 - 1
CHECKER = 0x55AA55AA55AA55AA


def _window(r, c, h, w):
    return sum(1 << ((r + i) * 8 + (c + j)) for i in range(h) for j in range(w))


def crafted_boards():
    """name -> u64 array: the empty, full and checker boards; every board with at most two filled cells and their
    complements; every single empty 3x3, 1x5 and 5x1 window in an otherwise full board."""
    few = [0] + [1 << a for a in range(64)] + [(1 << a) | (1 << b) for a in range(64) for b in range(a + 1, 64)]
    fam = {"basic": [0, FULL, CHECKER], "few": few, "few_complement": [FULL ^ b for b in few]}
    for name, (h, w) in (("window3x3", (3, 3)), ("window1x5", (1, 5)), ("window5x1", (5, 1))):
        fam[name] = [FULL ^ _window(r, c, h, w) for r in range(9 - h) for c in range(9 - w)]
    return {k: np.array(v, np.uint64) for k, v in fam.items()}


def random_boards(n, seed):
    """n seeded boards spread over all densities: board i has each cell filled with probability i / (n - 1)."""
    rng = np.random.default_rng(seed)
    p = np.linspace(0.0, 1.0, n)[:, None]
    cells = rng.random((n, 64)) < p
    return (cells.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def reference_terms():
    """(boards u64, terms int64 [n, 4], family slices) of the crafted families and 2,000 random boards, once."""
    fam = crafted_boards()
    fam["random"] = random_boards(2000, 20240607)
    boards = np.concatenate(list(fam.values()))
    where, lo = {}, 0
    for k, v in fam.items():
        where[k] = slice(lo, lo + len(v))
        lo += len(v)
    return boards, cell_terms(boards), where
