"""Shared by the tests of bb_playout_values (tests/test_playout_values_host.py, tests/test_gpu_playout_values.py and the
agent / tuner tests): two restatements of the dealt playouts, neither of which calls a bb_playout_* entry point.

* ``oracle``: include/bbvec.h "dealt playouts" in numpy and plain Python -- the deal from ``_refill_values_ref.deal``
  (the oracle's Philox, the C oracle's solvable search) under key (seed + h) mod 2^64, the search from
  ``_eval_terms_ref.chained_ext`` (a board that one move can empty goes through a recursion on the oracle env, as in
  tests/_values_ext_ref.py), the play through ``_play_plan_ref.oracle_play``.  A playout of H hands is a prefix of
  the same playout of more, so one run answers every hand count up to ``hands``.  It is slow: keep its sets tiny.
* ``composed``: the same over the *existing* entry points of one backend, per hand ``refill_values_ext`` on the n * m
  current boards with deals = m, element [pair, j] taken; ``plan_actions_ext`` for the plan; ``play_plan`` to advance.
  ``carry_combo=False`` is the mistake of resetting the combo between hands, for a test to show that its case can
  tell the two apart.

Both return the nine outputs of ``bb_playout_out``, each [n, playouts].
"""
import copy
import json
import os

import numpy as np
import torch

import _afterstates_ref as R
import _eval_terms_ref as E
import _play_plan_ref as PP
import _refill_values_ref as RV

OUTPUTS = ("value", "score", "lines", "plies", "hands", "status", "board", "combo", "hand")
DTYPES = {"value": np.int64, "score": np.int64, "lines": np.int32, "plies": np.int32, "hands": np.int32,
          "status": np.int32, "board": np.uint64, "combo": np.int32, "hand": np.uint32}
MASK64 = 2 ** 64 - 1
ZERO4 = {"perimeter": 0, "room3": 0, "room5": 0, "fits": 0}
PLAIN = {**R.DEFAULT_WEIGHTS, **ZERO4}
SHAPED = {**R.DEFAULT_WEIGHTS, **E.SETS["all"]}
SCORED = {**PLAIN, "score": 3}  # the combo shows in the score alone: a row that weighs it


def _oracle_plan(board, hand, combo, depth, w):
    """(value, plan [3], found) of one whole hand on the oracle env: every maximal sequence in lexicographic order,
    the first of the best kept."""
    O = E.P.O
    leaves = []  # (lines, score, features, board bits, sequence)

    def rec(env, d, lines, score, seq):
        for a in range(192):
            if not env.engine.can_place_piece(*O.Env.action_to_move(a)):
                continue
            refill = sum(env.engine.used) == 2
            cp = copy.deepcopy(env)
            if refill:  # the new hand and whether it fits are chance: left out
                cp.engine._generate = lambda: None
                cp.engine.has_valid_moves = lambda: True
            _, _, term, _, info = cp.step(a)
            sl = lines + info["last_move"]["lines_cleared"]
            ss = score + info["last_move"]["score_gained"]
            if d == 1 or refill or term:
                g = cp.engine.grid
                leaves.append((sl, ss, {"holes": O.count_holes(g), "centre": O.center_filled(g),
                                        "filled": O.total_blocks(g), "mobility": len(cp.engine.valid_moves()),
                                        "dead": int(term), "refill": int(refill)}, O.grid_to_u64(g), seq + [a]))
            else:
                rec(cp, d - 1, sl, ss, seq + [a])

    rec(RV._oracle_env(board, hand, combo), depth, 0, 0, [])
    if not leaves:
        return 0, [-1, -1, -1], False
    t = E.cell_terms(np.array([x[3] for x in leaves], np.uint64))
    v = [int(w.get("lines", 0)) * sl + int(w.get("score", 0)) * ss + sum(int(w.get(s, 0)) * f[s] for s in f)
         + sum(int(w.get(k, 0)) * int(t[x, j]) for j, k in enumerate(E.TERMS))
         for x, (sl, ss, f, _, _) in enumerate(leaves)]
    best = max(range(len(v)), key=lambda x: (v[x], -x))  # the first of the best
    seq = leaves[best][4]
    return v[best], seq + [-1] * (3 - len(seq)), True


def _search(boards, hands, combo, depth, ws):
    """(value [k], plan [k, 3], found [k]) of k positions with whole hands, position x under the dict ws[x]."""
    k = len(boards)
    value, plan, found = np.zeros(k, object), np.full((k, 3), -1, np.int64), np.zeros(k, bool)
    open_ = np.array([bin(int(b)).count("1") < RV.CROWDED_CELLS for b in boards], bool)
    sets = []
    for w in ws:
        if w not in sets:
            sets.append(w)
    which = np.array([sets.index(w) for w in ws])
    for s, w in enumerate(sets):
        idx = np.nonzero(open_ & (which == s))[0]
        if idx.size:
            res = E.chained_ext(boards[idx], hands[idx], combo[idx], depth, {"w": w})["w"]
            value[idx], plan[idx], found[idx] = res["value"], res["plan"], res["leaves"] > 0
    for x in np.nonzero(~open_)[0]:
        value[x], plan[x], found[x] = _oracle_plan(boards[x], hands[x], combo[x], depth, ws[x])
    return value, plan, found


def oracle(boards, weights, depth, playouts, hands, seed, combo=None, stream=None, carry_combo=True):
    """{H: the nine outputs as numpy [n, playouts]} for H = 1..hands.  ``weights``: one dict for all boards or a list
    of n dicts (board i's row)."""
    boards = np.asarray(boards, np.uint64)
    n, m = len(boards), int(playouts)
    ws = [weights] * n if isinstance(weights, dict) else list(weights)
    combo = np.zeros(n, np.int32) if combo is None else np.asarray(combo, np.int32)
    stream = np.arange(n, dtype=np.int64) if stream is None else np.asarray(stream, np.int64)
    owner, deal_j = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
    B, cb = boards[owner].copy(), combo[owner].astype(np.int64)
    moved = np.zeros(n * m, object)
    st = {k: np.zeros(n * m, object) for k in ("value", "score", "lines", "plies", "hands", "status", "hand")}
    live = np.ones(n * m, bool)
    out = {}
    for h in range(int(hands)):
        idx = np.nonzero(live)[0]
        if idx.size:
            key = (int(seed) + h) & MASK64
            dealt = RV.deal(B[idx], m, key, stream[owner[idx]])[0][np.arange(idx.size), deal_j[idx]]
            value, plan, found = _search(B[idx], dealt, cb[idx], depth, [ws[owner[x]] for x in idx])
            for t, x in enumerate(idx):
                w = ws[owner[x]]
                st["hand"][x], st["hands"][x] = int(dealt[t]), h + 1
                if not found[t]:  # no legal first move: nothing is played
                    st["value"][x], st["status"][x], live[x] = moved[x] + int(w.get("dead", 0)), 0, False
                    continue
                st["value"][x] = moved[x] + int(value[t])
                ids = [(int(dealt[t]) >> (6 * p)) & 63 for p in range(3)]
                leaf = PP.oracle_play(R.make_env(int(B[x]), ids, combo=int(cb[x])), [int(a) for a in plan[t]])
                B[x], cb[x] = leaf[0], leaf[2] if carry_combo else 0
                st["lines"][x] += leaf[3]
                st["score"][x] += leaf[4]
                st["plies"][x] += leaf[5] & PP.PLIES
                st["status"][x] = leaf[5]
                m_h = int(w.get("lines", 0)) * leaf[3] + int(w.get("score", 0)) * leaf[4]
                if leaf[5] & PP.REFILL:
                    moved[x] += m_h
                else:
                    live[x] = False
        snap = {k: np.array([int(v) for v in st[k]], DTYPES[k]).reshape(n, m) for k in st}
        snap["board"], snap["combo"] = B.copy().reshape(n, m), cb.astype(np.int32).reshape(n, m)
        out[h + 1] = snap
    return out


def composed(board, rows, depth, playouts, hands, seed, combo=None, stream=None, carry_combo=True):
    """The nine outputs as tensors [n, playouts], from refill_values_ext + plan_actions_ext + play_plan where the
    tensors live.  rows: int32 [1, 12] or [n, 12]."""
    from runtime import kernels as K

    n, m, dev = board.numel(), int(playouts), board.device
    combo = torch.zeros(n, dtype=torch.int32, device=dev) if combo is None else combo
    stream = torch.arange(n, dtype=torch.int64, device=dev) if stream is None else stream
    owner = torch.arange(n, device=dev).repeat_interleave(m)
    pair = torch.arange(n * m, device=dev)
    deal_j = pair % m
    each = (rows if rows.shape[0] == n and n > 1 else rows[:1].expand(n, 12))[owner].contiguous()
    B, cb, sid = board[owner].contiguous(), combo[owner].contiguous(), stream[owner].contiguous()
    z64 = lambda: torch.zeros(n * m, dtype=torch.int64, device=dev)  # noqa: E731
    z32 = lambda: torch.zeros(n * m, dtype=torch.int32, device=dev)  # noqa: E731
    moved, value, score, lines, plies, searched, status, last = z64(), z64(), z64(), z32(), z32(), z32(), z32(), z32()
    live = torch.ones(n * m, dtype=torch.bool, device=dev)
    lowest = torch.iinfo(torch.int64).min
    for h in range(int(hands)):
        key = (int(seed) + h) & MASK64
        rv = K.refill_values_ext(B, each, m, key, combo=cb, stream=sid, depth=depth, want=("hand", "value"))
        dealt, v = rv["hand"][pair, deal_j].contiguous(), rv["value"][pair, deal_j]
        pl = K.plan_actions_ext(B, dealt, each, depth, combo=cb, want_plan=True)
        found = pl["value"] != lowest
        assert torch.equal(torch.where(found, pl["value"], each[:, 6].long()), v)  # the two searches agree
        leaf = K.play_plan(B, dealt, pl["plan"].contiguous(), cb)
        refill = (leaf["status"] & K.PLAY_REFILL) != 0
        value = torch.where(live, moved + v, value)
        last = torch.where(live, dealt, last)
        searched = torch.where(live, torch.full_like(searched, h + 1), searched)
        status = torch.where(live, leaf["status"], status)
        score = torch.where(live, score + leaf["score"], score)
        lines = torch.where(live, lines + leaf["lines"], lines)
        plies = torch.where(live, plies + (leaf["status"] & K.PLAY_PLIES), plies)
        B = torch.where(live, leaf["board"], B).contiguous()
        cb = torch.where(live, leaf["combo"] if carry_combo else torch.zeros_like(cb), cb).contiguous()
        moved = moved + torch.where(live & refill, each[:, 0].long() * leaf["lines"] + each[:, 1].long() * leaf["score"], 0)
        live = live & found & refill
    res = {"value": value, "score": score, "lines": lines, "plies": plies, "hands": searched, "status": status,
           "board": B, "combo": cb, "hand": last}
    return {k: t.view(n, m) for k, t in res.items()}


def as_numpy(out):
    """The outputs as numpy arrays of the C types (board u64, hand u32)."""
    res = {}
    for k, v in out.items():
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        res[k] = a.view(DTYPES[k]) if a.dtype.itemsize == np.dtype(DTYPES[k]).itemsize else a.astype(DTYPES[k])
    return res


def assert_equal(got, want, what=""):
    got, want = as_numpy(got), as_numpy(want)
    for key in OUTPUTS:
        if key in got:
            bad = np.argwhere(got[key] != want[key].reshape(got[key].shape))[:6]
            assert bad.size == 0, (what, key, bad.tolist(), [got[key][tuple(b)].item() for b in bad],
                                   [want[key][tuple(b)].item() for b in bad])


def endings(want):
    """(survived, dead leaf, cut short, no legal first move) playouts of a reference answer."""
    st = as_numpy(want)["status"]
    return (int(((st & PP.REFILL) != 0).sum()), int(((st & PP.DEAD) != 0).sum()),
            int(((st != 0) & (st & (PP.REFILL | PP.DEAD) == 0)).sum()), int((st == 0).sum()))


def call(board, rows, depth, playouts, hands, seed, combo=None, stream=None, want=OUTPUTS, **kw):
    from runtime import kernels as K

    return K.playout_values(board, rows, playouts, hands, seed, combo=combo, stream=stream, depth=depth, want=want,
                            **kw)


def guarded(n, playouts, dev, key, word=0x5A):
    """An output tensor of bb_playout_out between two guard blocks of 64 bytes: (whole uint8 buffer, the view)."""
    from runtime import kernels as K

    dt = K.PLAYOUT_OUTPUTS[key]
    size = n * playouts * torch.empty(0, dtype=dt).element_size()
    buf = torch.full((size + 128,), word, dtype=torch.uint8, device=dev)
    return buf, buf[64:64 + size].view(dt).view(n, playouts)


def guards_intact(buf, word=0x5A):
    return bool((buf[:64] == word).all()) and bool((buf[-64:] == word).all())


def board_tensor(bs, dev="cpu"):
    return RV.board_tensor(bs, dev)


def rows_of(ws, dev="cpu"):
    from runtime import kernels as K

    return torch.cat([K.eval_rows(w) for w in ([ws] if isinstance(ws, dict) else ws)]).contiguous().to(dev)


# ---- the tiny fixed case of the oracle tests (host and GPU): five boards, eight playouts, up to three hands ---------
# Crowded boards, so that the depth-3 trees stay small and the dealer refuses: the checker (dead leaves and hands with
# no legal first move at hand 1, one playout that lives on), the checker with row 7 empty under a row that plays to
# fill the board (a dead leaf at hand 2), the full board (nothing is ever legal), the board with one hole (one move
# can clear 16 lines: the oracle-env recursion) and a dense board of the census set.  Rows of both kinds, stream ids
# shared by two boards, combos carried in.
ANTI = {**ZERO4, "lines": -100, "score": 0, "holes": 30, "filled": 50, "centre": 0, "mobility": -1, "dead": -100000,
        "refill": 0}
TINY_SEED, TINY_PLAYOUTS, TINY_HANDS, TINY_DEPTH = 11, 8, 3, 3
TINY_STREAM = np.array([2, 1, 9, 3, 3], np.int64)
TINY_COMBO = np.array([0, 2, 0, 4, 1], np.int32)
TINY_WEIGHTS = [PLAIN, ANTI, SHAPED, SCORED, SHAPED]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "playout_tiny.json")


def tiny_boards():
    import _census_ref as C

    return np.array([C.CHECKER, C.CHECKER_ROW7_EMPTY, C.FULL, C.ONE_HOLE, int(C.boards()[7])], np.uint64)


def tiny_oracle():
    """The oracle on the tiny case at depth 3 (half a minute): {H: outputs} for H = 1..3."""
    return oracle(tiny_boards(), TINY_WEIGHTS, TINY_DEPTH, TINY_PLAYOUTS, TINY_HANDS, TINY_SEED, combo=TINY_COMBO,
                  stream=TINY_STREAM)


def tiny_golden():
    """The oracle's answer on the tiny case as recorded in tests/golden/playout_tiny.json ({H: outputs}; the boards
    it was recorded for are checked).  tests/test_playout_values_host.py holds the file to ``tiny_oracle`` itself, so
    the quick tests of both backends can read it instead of searching for half a minute."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["boards"] == [int(b) for b in tiny_boards()] and doc["seed"] == TINY_SEED
    return {int(h): {k: np.array(v, object).astype(DTYPES[k]) for k, v in o.items()} for h, o in doc["hands"].items()}


def write_tiny_golden():
    res = tiny_oracle()
    doc = {"boards": [int(b) for b in tiny_boards()], "seed": TINY_SEED,
           "hands": {str(h): {k: [[int(x) for x in row] for row in v] for k, v in o.items()} for h, o in res.items()}}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f)
    return res


def tiny_tensors(dev):
    """(board, rows, combo, stream) of the tiny case on ``dev``."""
    return (board_tensor(tiny_boards(), dev), rows_of(TINY_WEIGHTS, dev), torch.from_numpy(TINY_COMBO.copy()).to(dev),
            torch.from_numpy(TINY_STREAM.copy()).to(dev))
