"""Shared by the tests of bb_plan2_values (tests/test_plan2_values_host.py, tests/test_gpu_plan2_values.py and the
agent / tuner tests): two restatements of the two-hand decision, neither of which calls a bb_plan2_* entry point.

* ``oracle``: steps 1-6 of include/bbvec.h in numpy and plain Python -- q and rest from
  ``_values_ext_ref.per_action_ext``, a stable descending sort, every candidate's leaf from the oracle env
  (``_play_plan_ref.oracle_play``), the dealt hands and their values from ``_values_ext_ref.refill_values_ext``
  (``_refill_values_ref.deal`` + ``chained_ext``).  It is slow: keep its position sets small.
* ``composed``: the same steps over the *existing* entry points of one backend (``plan_values_ext``, ``play_plan``,
  ``refill_values_ext``, each pinned to the oracle by its own tests) with ``TwoHandPlanAgent._decide``'s torch steps
  in between, for the larger sets and for the GPU.

Both return the five outputs of ``bb_plan2_out``: action i32 [n], q2 i64 [n, 192], cand i32 [n, K], status i32
[n, K], value i64 [n, K, deals].
"""
import numpy as np
import torch

import _afterstates_ref as R
import _play_plan_ref as PP
import _values_ext_ref as X

INT64_MIN = R.INT64_MIN
OUTPUTS = ("action", "q2", "cand", "status", "value")
ZERO12 = {k: 0 for k in ("lines", "score", "holes", "filled", "centre", "mobility", "dead", "refill", "perimeter",
                         "room3", "room5", "fits")}
SHAPED = {**R.DEFAULT_WEIGHTS, **X.SETS["all"]}
PLAIN = {**R.DEFAULT_WEIGHTS, "perimeter": 0, "room3": 0, "room5": 0, "fits": 0}


def oracle(board, hand, combo, weights, depth, k, deals, seed, stream=None):
    """``weights``: one dict for all positions or a list of n dicts (position i's row)."""
    board, hand = np.asarray(board, np.uint64), np.asarray(hand, np.uint32)
    n = len(board)
    combo = np.zeros(n, np.int32) if combo is None else np.asarray(combo, np.int32)
    ws = [weights] * n if isinstance(weights, dict) else list(weights)
    stream = np.arange(n, dtype=np.int64) if stream is None else np.asarray(stream, np.int64)
    sets = []
    for w in ws:
        if w not in sets:
            sets.append(w)
    which = np.array([sets.index(w) for w in ws])
    out = {"action": np.zeros(n, np.int32), "q2": np.full((n, 192), INT64_MIN, np.int64),
           "cand": np.full((n, k), -1, np.int32), "status": np.full((n, k), -1, np.int32),
           "value": np.zeros((n, k, deals), np.int64)}
    for s, w in enumerate(sets):
        idx = np.nonzero(which == s)[0]
        per = X.per_action_ext(board[idx], hand[idx], combo[idx], depth, {"w": w})          # step 1
        q, rest = per["q"]["w"], per["rest"]["w"]
        assert ((q != INT64_MIN) == per["legal"]).all()
        leaves = []  # (position, rank, action, leaf)
        for t, i in enumerate(idx):
            order = np.argsort(-q[t].astype(object), kind="stable")                          # step 2
            for r, a in enumerate([int(a) for a in order if q[t, a] != INT64_MIN][:k]):
                a2, a3 = int(rest[t, a]) & 0xFF, (int(rest[t, a]) >> 8) & 0xFF
                h = int(hand[i])
                env = R.make_env(int(board[i]), [(h >> (6 * p)) & 63 for p in range(3)],
                                 used=[bool((h >> (18 + p)) & 1) for p in range(3)], combo=int(combo[i]))
                leaf = PP.oracle_play(env, [a, -1 if a2 == 0xFF else a2, -1 if a3 == 0xFF else a3])  # step 3
                leaves.append((i, r, a, leaf))
                out["cand"][i, r], out["status"][i, r] = a, leaf[5]
                out["q2"][i, a] = deals * int(q[t, a])                                        # step 5
        refills = [x for x in leaves if x[3][5] & PP.REFILL]
        if refills:                                                                          # step 4
            ref = X.refill_values_ext(np.array([x[3][0] for x in refills], np.uint64), deals, seed, depth, {"w": w},
                                      combo=[x[3][2] for x in refills], stream=[int(stream[x[0]]) for x in refills])
            for (i, r, a, leaf), values in zip(refills, ref["value"]["w"]):
                moved = int(w.get("lines", 0)) * leaf[3] + int(w.get("score", 0)) * leaf[4]
                out["value"][i, r] = values
                out["q2"][i, a] = deals * moved + int(values.sum())
    for i in range(n):                                                                       # step 6
        cands = [int(a) for a in out["cand"][i] if a >= 0]
        if cands:
            best = max(int(out["q2"][i, a]) for a in cands)
            out["action"][i] = min(a for a in cands if int(out["q2"][i, a]) == best)
    return out


def composed(board, hand, combo, rows, depth, k, deals, seed, stream=None, deal_combo="leaf"):
    """The five outputs as tensors, from plan_values_ext + play_plan + refill_values_ext where the tensors live.
    rows: int32 [1, 12] or [n, 12].  ``deal_combo="root"`` is the mistake of dealing under the root's combo, for a
    test to show that its case can tell the two apart."""
    from runtime import kernels as K

    n, dev = board.numel(), board.device
    combo = torch.zeros(n, dtype=torch.int32, device=dev) if combo is None else combo
    root = torch.arange(n, dtype=torch.int64, device=dev)
    stream = root if stream is None else stream
    each = rows if rows.shape[0] == n else rows.expand(n, 12)
    pv = K.plan_values_ext(board, hand, rows, depth, combo=combo, want=("q", "rest"))
    q, rest = pv["q"], pv["rest"]
    lowest = torch.iinfo(torch.int64).min
    kk = min(k, 192)
    cand = torch.sort(q, dim=1, descending=True, stable=True).indices[:, :kk]
    qc = q.gather(1, cand)
    valid = qc != lowest
    a2, a3 = K.unpack_rest(rest.gather(1, cand))
    plan = torch.stack([cand.to(torch.int32), a2.to(torch.int32), a3.to(torch.int32)], dim=2)
    plan = torch.where(valid.unsqueeze(2), plan, torch.full_like(plan, -1)).view(n * kk, 3).contiguous()
    leaf = K.play_plan(board.repeat_interleave(kk), hand.repeat_interleave(kk), plan, combo.repeat_interleave(kk),
                       want=("board", "combo", "lines", "score", "status"))
    flat_valid = valid.reshape(-1)
    refill = ((leaf["status"] & K.PLAY_REFILL) != 0) & flat_valid
    q2c = torch.where(valid, deals * qc, torch.full_like(qc, lowest)).reshape(-1)
    value = torch.zeros((n * kk, deals), dtype=torch.int64, device=dev)
    idx = torch.nonzero(refill).view(-1)
    if idx.numel():
        owner = root.repeat_interleave(kk)[idx]
        v = K.refill_values_ext(leaf["board"][idx].contiguous(), each[owner].contiguous(), deals, seed,
                                combo=(leaf["combo"] if deal_combo == "leaf" else combo.repeat_interleave(kk))[idx]
                                .contiguous(), stream=stream[owner].contiguous(),
                                depth=depth)["value"]
        w = each[owner].long()
        moved = w[:, 0] * leaf["lines"][idx].long() + w[:, 1] * leaf["score"][idx]
        value[idx] = v
        q2c[idx] = deals * moved + v.sum(dim=1)
    q2c = q2c.view(n, kk)
    best = q2c.max(dim=1, keepdim=True).values
    action = torch.where((q2c == best) & valid, cand, torch.full_like(cand, 192)).min(dim=1).values
    action = torch.where(valid.any(dim=1), action, torch.zeros_like(action)).to(torch.int32)
    q2 = torch.full((n, 192), lowest, dtype=torch.int64, device=dev)
    q2.scatter_(1, cand, q2c)  # an absent candidate scatters INT64_MIN onto an illegal action
    return {"action": action, "q2": q2, "cand": torch.where(valid, cand, -1).to(torch.int32),
            "status": torch.where(valid, leaf["status"].view(n, kk), -1).to(torch.int32),
            "value": value.view(n, kk, deals)}


def as_numpy(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}


def assert_equal(got, want, what=""):
    got, want = as_numpy(got), as_numpy(want)
    for key in OUTPUTS:
        if key in got:
            g, w = got[key], want[key].reshape(got[key].shape)
            bad = np.nonzero(np.atleast_1d((g != w).reshape(len(g), -1).any(axis=1)))[0] if len(g) else []
            assert len(bad) == 0, f"{what} {key}: positions {list(bad)[:8]} differ"


def leaf_kinds(want):
    """(refill, dead, cut) candidates of a reference answer: counts by the leaf's status word."""
    st = as_numpy(want)["status"]
    present = st >= 0
    refill = present & ((st & PP.REFILL) != 0)
    dead = present & ((st & PP.DEAD) != 0)
    return int(refill.sum()), int(dead.sum()), int((present & ~refill & ~dead).sum())


def call(board, hand, combo, rows, depth, k, deals, seed, stream=None, want=OUTPUTS, **kw):
    from runtime import kernels as K

    return K.plan2_values(board, hand, rows, k, deals, seed, combo=combo, stream=stream, depth=depth, want=want, **kw)


def guarded(n, k, deals, dev, key, word=0x5A):
    """An output tensor of bb_plan2_out between two guard blocks of 64 bytes: (whole uint8 buffer, the view)."""
    from runtime import kernels as K

    dt = K.PLAN2_OUTPUTS[key]
    shape = {"action": (n,), "q2": (n, 192), "cand": (n, k), "status": (n, k), "value": (n, k, deals)}[key]
    size = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
    buf = torch.full((size + 128,), word, dtype=torch.uint8, device=dev)
    return buf, buf[64:64 + size].view(dt).view(shape)


def guards_intact(buf, word=0x5A):
    return bool((buf[:64] == word).all()) and bool((buf[-64:] == word).all())


# ---- position sets -----------------------------------------------------------------------------------------------
def _hand(a, b, c, used=0, over=False):
    return a | b << 6 | c << 12 | used << 18 | int(over) << 21


def crafted():
    """name -> (board, hand, combo): the positions built so that a condition of the contract holds by construction."""
    row_short = sum(1 << c for c in range(7))              # row 0 one cell short: the SINGLE at cell 7 clears it
    return {
        "empty_singles": (0, _hand(0, 0, 0), 0),            # 192 legal actions at depth 1
        "game_over_bit": (0, _hand(0, 1, 2, over=True), 0),   # nothing is legal
        "all_used": (0, _hand(0, 1, 2, used=7), 0),           # nothing is legal
        "full_but_one": (0xFFFFFFFFFFFFFFFF ^ (1 << 27) ^ (1 << 36), _hand(36, 36, 36), 0),  # the 3x3 fits nowhere
        "one_slot_left": (0x00000000000F0F0F, _hand(5, 6, 0, used=3), 2),  # every move is a refill
        "combo5_row_short": (row_short, _hand(1, 2, 0, used=3), 5),    # the clearing leaf carries combo 6
        "whole_hand": (0x0000001818000000, _hand(5, 9, 1), 1),
        # column 0 one cell short, the SINGLE left: under {"lines": 1} the clearing move (action 184) ranks first, and a
        # move elsewhere ties with it in Q2 whenever the dealt hand can finish the column
        "col_short": (sum(1 << (r * 8) for r in range(7)), _hand(1, 2, 0, used=3), 0),
    }


def positions():
    """(board u64, hand u32, combo i32, names {name: index}): the played and crafted positions of
    tests/_afterstates_ref.py, 46 crowded ones of tests/_safe_positions.py and ``crafted`` above."""
    import _safe_positions as S

    ref = R.reference()
    cb, ch = S.crowded(n=420)
    pick = np.arange(0, 420, 9)[:46]
    made = crafted()
    board = np.concatenate([ref["board"], cb[pick], np.array([v[0] for v in made.values()], np.uint64)])
    hand = np.concatenate([ref["hand"], ch[pick], np.array([v[1] for v in made.values()], np.uint32)])
    combo = np.concatenate([ref["combo"].astype(np.int32), (np.arange(len(pick)) % 4).astype(np.int32),
                            np.array([v[2] for v in made.values()], np.int32)])
    names = {k: len(board) - len(made) + j for j, k in enumerate(made)}
    return board, hand, combo, names


def to_tensors(board, hand, combo, dev, idx=None):
    sel = slice(None) if idx is None else idx
    return (torch.from_numpy(np.asarray(board, np.uint64)[sel].view(np.int64).copy()).to(dev),
            torch.from_numpy(np.asarray(hand, np.uint32)[sel].view(np.int32).copy()).to(dev),
            torch.from_numpy(np.asarray(combo, np.int32)[sel].copy()).to(dev))


def mixed_rows(n, dev):
    """int32 [n, 12]: shaped, zero-shape and all-zero rows in turn, so one launch runs both sides of the branch."""
    from runtime import kernels as K

    kinds = [K.eval_rows(w)[0] for w in (SHAPED, PLAIN, ZERO12, {**SHAPED, "lines": 300, "holes": -5})]
    return torch.stack([kinds[i % 4] for i in range(n)]).contiguous().to(dev)


# ---- the agents' games ---------------------------------------------------------------------------------------------
def play(agent, seeds, moves, device="cpu"):
    """The actions of ``moves`` decisions of ``agent`` on the games of ``seeds``: a list of lists."""
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(len(seeds), list(seeds), autoreset=False, device=device)
    env.reset()
    act = torch.zeros(len(seeds), dtype=torch.int32, device=env.device)
    log = []
    for _ in range(moves):
        agent.act_env(env, act)
        log.append(act.tolist())
        env.step(act)
    env.close()
    return log


def population(weights, n, device="cpu", **kw):
    """``PopulationTwoHandAgent`` of n envs under one weight dict, or under a list of n."""
    from agents import PopulationTwoHandAgent
    from runtime import kernels as K

    rows = torch.cat([K.eval_rows(w) for w in (weights if isinstance(weights, list) else [weights] * n)])
    return PopulationTwoHandAgent(rows, device=device, **kw)
