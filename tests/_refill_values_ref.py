"""Shared by the dealt-next-hand tests (tests/test_refill_values_host.py, tests/test_gpu_refill_values.py,
tests/test_two_hand_agent_host.py): a reference for bb_refill_values that calls none of its entry points.

* the dealer (include/bbvec.h "dealt next-hand values"; engine.py:155-172) restated with the oracle's Philox
  (``oracle.philox.philox4x32_10``) and the C oracle's depth-first search (``oracle.c_oracle.solvable_many``);
* the value restated with tests/_plan_ref.py's searches, a hand without a legal first move priced at the ``dead``
  weight: the level-by-level ``chained``, and on boards that one move can empty its recursion on the oracle env,
  ``oracle_search`` (``chained`` reads a move's lines from an aux word that has four bits for them; 16 do not fit).

The fixed case: seed 1, stream = i, 8 deals on five named boards.  The coverage the tests rely on is asserted here
from the oracle's answers alone, so that a change of the contract cannot silently empty a class.
"""
import functools

import numpy as np
import torch

import _plan_ref as P

ATTEMPTS = 100
FIXED_BOARDS = np.array([0, 0xFFFFFFFFFFFFFFFF, 0x55AA55AA55AA55AA, 0x00AA55AA55AA55AA, 0xFFFFFFFFF7FFFFFF], np.uint64)
EMPTY, FULL, CHECKER, CHECKER_ROW7_EMPTY, ONE_HOLE = range(5)
FIXED_SEED, FIXED_DEALS = 1, 8
WEIGHTS = P.WEIGHT_SETS["default"]


def deal(boards, deals, seed, stream=None):
    """(hand u32 [n, deals], attempts i32 [n, deals]) of the dealer on the boards (u64 [n])."""
    from oracle import c_oracle
    from oracle.philox import philox4x32_10

    boards = np.asarray(boards, np.uint64)
    n = len(boards)
    idx = np.arange(n, dtype=np.uint64) if stream is None else np.asarray(stream).astype(np.uint64)
    hands = np.zeros((n, deals, ATTEMPTS), np.uint32)
    for j in range(deals):
        for t in range(ATTEMPTS):
            w = philox4x32_10(idx, (j << 7) | t, seed)
            a, b, c = ((w[k].astype(np.uint64) * np.uint64(37)) >> np.uint64(32) for k in range(3))
            hands[:, j, t] = (a | b << np.uint64(6) | c << np.uint64(12)).astype(np.uint32)
    ok = c_oracle.solvable_many(np.repeat(boards, deals * ATTEMPTS), hands.reshape(-1)).reshape(n, deals, ATTEMPTS)
    first = ok.argmax(axis=2)
    accepted = ok.any(axis=2)
    pick = np.where(accepted, first, ATTEMPTS - 1)
    hand = np.take_along_axis(hands, pick[:, :, None], axis=2)[:, :, 0]
    return hand, np.where(accepted, first + 1, -ATTEMPTS).astype(np.int32)


CROWDED_CELLS = 55  # a move can clear all 16 lines only on a board with 64 - 9 cells or more


def _oracle_env(board, hand, combo):
    """An oracle env standing on (board, whole hand, combo)."""
    from oracle import bb_game as O

    env = O.Env(seed=0)
    env.engine.grid = [[(int(board) >> (r * 8 + c)) & 1 for c in range(8)] for r in range(8)]
    env.engine.hand = [(int(hand) >> (6 * s)) & 63 for s in range(3)]
    env.engine.used = [False, False, False]
    env.engine.combo = int(combo)
    return env


def search(boards, hands, combo, depth, weights):
    """(value i64 [n, deals], leaves [n, deals]) of the dealt hands (u32 [n, deals]) on their boards at combo [n].
    ``P.chained`` reads the lines of a move from the one-ply call's aux word, which has four bits for them: a board
    that one move can empty (16 lines) goes through ``P.oracle_search`` instead, whose trees are small there."""
    boards = np.asarray(boards, np.uint64)
    n, m = hands.shape
    combo = np.zeros(n, np.int32) if combo is None else np.asarray(combo, np.int32)
    value, leaves = np.zeros((n, m), np.int64), np.zeros((n, m), np.int64)
    open_ = np.array([bin(int(b)).count("1") < CROWDED_CELLS for b in boards])
    if open_.any():
        res = P.chained(np.repeat(boards[open_], m), hands[open_].reshape(-1).astype(np.uint32),
                        np.repeat(combo[open_], m), depth, {"w": weights})["w"]
        value[open_], leaves[open_] = res["value"].reshape(-1, m), res["leaves"].reshape(-1, m)
    for i in np.nonzero(~open_)[0]:
        for j in range(m):
            value[i, j], _, leaves[i, j] = P.oracle_search(_oracle_env(boards[i], hands[i, j], combo[i]), depth, weights)
    return np.where(leaves == 0, np.int64(weights.get("dead", 0)), value), leaves


def refill_values(boards, deals, seed, depth, weights=WEIGHTS, combo=None, stream=None):
    """{"hand" u32, "value" i64, "attempts" i32, "leaves"}, each [n, deals]: the whole call restated."""
    hand, attempts = deal(boards, deals, seed, stream)
    value, leaves = search(boards, hand, combo, depth, weights)
    return {"hand": hand, "value": value, "attempts": attempts, "leaves": leaves}


@functools.lru_cache(maxsize=None)
def fixed(depth):
    """The fixed case at ``depth`` with its coverage asserted (the attempts do not depend on the depth)."""
    ref = refill_values(FIXED_BOARDS, FIXED_DEALS, FIXED_SEED, depth)
    at, leaves = ref["attempts"], ref["leaves"]
    assert (at[EMPTY] == 1).all()                                       # accepted at once
    assert at[CHECKER_ROW7_EMPTY][:3].tolist() == [8, 22, 48] and at[ONE_HOLE][:3].tolist() == [17, 25, 49]
    assert ((at[[CHECKER_ROW7_EMPTY, ONE_HOLE]] > 1) & (at[[CHECKER_ROW7_EMPTY, ONE_HOLE]] < ATTEMPTS)).sum() >= 6
    assert (at[FULL] == -ATTEMPTS).all() and (leaves[FULL] == 0).all()  # refused, and no legal first move
    assert at[CHECKER][1] == -ATTEMPTS and leaves[CHECKER][1] == 0
    assert at[CHECKER][0] == -ATTEMPTS and leaves[CHECKER][0] > 0       # refused, a first move, dead leaves only
    assert at[CHECKER][3] == 48 and at[CHECKER][5] == 25                # accepted late in the loop
    for v in ref.values():
        v.setflags(write=False)
    return ref


def board_tensor(bs, dev="cpu"):
    return torch.from_numpy(np.asarray(bs, np.uint64).view(np.int64).copy()).to(dev)


def as_u32(t):
    return t.detach().cpu().numpy().view(np.uint32)
