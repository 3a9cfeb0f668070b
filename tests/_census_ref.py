"""Shared by the refill-census tests (tests/test_refill_census_host.py, tests/test_gpu_refill_census.py,
tests/test_census_tune_host.py, tests/test_gpu_census_tune.py): the 9,139 multisets of three pieces, the reference set
of boards and ``oracle_census``, the census through the C oracle's depth-first search (oracle.c_oracle.solvable_many,
one call per (board, multiset)).  Nothing here calls bb_refill_census or anything built on it.
"""
import functools
import itertools

import numpy as np
import torch

import _safe_positions as S

NP = 37
NUM_HANDS = NP ** 3  # 50,653

MULTISETS = np.array(list(itertools.combinations_with_replacement(range(NP), 3)), np.int64)  # [9139, 3], a <= b <= c
assert len(MULTISETS) == 9139
HAND_WORDS = (MULTISETS[:, 0] | MULTISETS[:, 1] << 6 | MULTISETS[:, 2] << 12).astype(np.uint32)
# ordered hands per multiset: 6 (all different), 3 (two equal), 1 (all equal)
MULTIPLICITY = np.array([{3: 6, 2: 3, 1: 1}[len(set(m))] for m in MULTISETS.tolist()], np.int64)
assert int(MULTIPLICITY.sum()) == NUM_HANDS

EMPTY, FULL = 0, 2 ** 64 - 1
CHECKER, CHECKER_ROW7_EMPTY, ONE_HOLE = 0x55AA55AA55AA55AA, 0x00AA55AA55AA55AA, 0xFFFFFFFFF7FFFFFF
NAMED = {"empty": (EMPTY, 50653), "full": (FULL, 0), "checker": (CHECKER, 125),
         "checker_row7_empty": (CHECKER_ROW7_EMPTY, 2995), "one_hole": (ONE_HOLE, 3997)}


def _fill(b):
    return bin(int(b)).count("1") / 64.0


def _played(seeds=(3, 5, 8, 13), moves=(5, 30, 100)):
    """Boards of games on the host backend under the depth-2 full-hand search, taken after `moves` moves."""
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime.build import build_host_lib
    from runtime.device_env import DeviceEnvBatch

    build_host_lib(verbose=False)
    env = DeviceEnvBatch(len(seeds), list(seeds), autoreset=False, device="cpu")
    env.reset()
    act = torch.zeros(len(seeds), dtype=torch.int32)
    out = []
    for t in range(1, max(moves) + 1):
        env.plan_actions(act, DEFAULT_WEIGHTS, depth=2)
        env.step(act)
        if t in moves:
            st = env.state()
            out += [int(b) for b, h in zip(st["board"], st["hand"]) if not (int(h) >> 21) & 1]
    env.close()
    return out


@functools.lru_cache(maxsize=None)
def boards():
    """The reference set, u64 [n]: the five named boards first (in NAMED's order), ten crowded boards at fill >= 0.6,
    nine at fill <= 0.5, and boards of played games after 5, 30 and 100 moves."""
    crowded, _ = S.crowded()
    dense = [int(b) for b in crowded if _fill(b) >= 0.6][:10]
    sparse = [int(b) for b in crowded if _fill(b) <= 0.5][:9]
    assert len(dense) >= 8 and len(sparse) >= 8
    played = _played()
    assert len(played) >= 9
    out = np.array([b for b, _ in NAMED.values()] + dense + sparse + played, np.uint64)
    out.setflags(write=False)
    return out


def solvable_words(flags):
    """bool [n, 9139] (one flag per multiset) -> u64 [n, 37, 37], bit c of word [a, b] for every permutation."""
    n = flags.shape[0]
    words = np.zeros((n, NP, NP), np.uint64)
    for perm in itertools.permutations(range(3)):
        a, b, c = (MULTISETS[:, k] for k in perm)
        for i in range(n):
            np.bitwise_or.at(words[i], (a[flags[i]], b[flags[i]]), np.uint64(1) << c[flags[i]].astype(np.uint64))
    return words


def oracle_flags(bs):
    """bool [n, 9139]: engine.py:174-224 through the C oracle for every (board, multiset)."""
    from oracle import c_oracle

    bs = np.asarray(bs, np.uint64)
    rep = np.repeat(bs, len(MULTISETS))
    hands = np.tile(HAND_WORDS, len(bs))
    return c_oracle.solvable_many(rep, hands).reshape(len(bs), len(MULTISETS))


_CACHE = {}


def oracle_census(bs):
    """(count i64 [n], solvable u64 [n, 37, 37]) of the boards, every board's answer cached by its value."""
    bs = np.asarray(bs, np.uint64)
    todo = sorted({int(b) for b in bs} - set(_CACHE))
    if todo:
        flags = oracle_flags(np.array(todo, np.uint64))
        words = solvable_words(flags)
        for k, b in enumerate(todo):
            w = words[k]
            w.setflags(write=False)
            _CACHE[b] = (int((flags[k] * MULTIPLICITY).sum()), w)
    count = np.array([_CACHE[int(b)][0] for b in bs], np.int64)
    words = np.stack([_CACHE[int(b)][1] for b in bs]) if len(bs) else np.zeros((0, NP, NP), np.uint64)
    return count, words


def fits(board):
    """bool [37]: piece p has a free anchor on the board (board.py:71-93 over every anchor, from the piece shapes)."""
    from game.pieces import PIECE_LIST

    out = np.zeros(NP, bool)
    for k, p in enumerate(PIECE_LIST):
        out[k] = any(not (int(board) & (p.bits << (r * 8 + c)))
                     for r in range(9 - p.height) for c in range(9 - p.width))
    return out


def needs_clear(board, words):
    """Some solvable hand of the board (words u64 [37, 37]) has a member that does not fit the board itself, so a
    line has to be cleared before it goes down."""
    f = fits(board)
    for a in np.nonzero(~f)[0]:  # the solvable hands that hold a: row a of the words
        if words[a].any():
            return True
    return False


@functools.lru_cache(maxsize=None)
def reference():
    """{"board" u64 [n], "count" i64 [n], "solvable" u64 [n, 37, 37]} of the reference set, with the coverage the
    tests rely on asserted from the oracle's answer alone."""
    bs = boards()
    count, words = oracle_census(bs)
    for k, (name, (b, want)) in enumerate(NAMED.items()):
        assert int(bs[k]) == b and int(count[k]) == want, (name, int(count[k]), want)
    p = count / NUM_HANDS
    assert (count == 0).any() and (count == NUM_HANDS).any()
    assert ((p > 0) & (p < 0.01)).sum() >= 1 and ((p >= 0.01) & (p < 0.1)).sum() >= 1
    assert ((p >= 0.1) & (p < 0.5)).sum() >= 3 and ((p >= 0.5) & (p < 1)).sum() >= 3, np.round(p, 3).tolist()
    assert any(needs_clear(int(b), words[k]) for k, b in enumerate(bs))
    count.setflags(write=False)
    words.setflags(write=False)
    return {"board": bs, "count": count, "solvable": words}


def board_tensor(bs, dev="cpu"):
    return torch.from_numpy(np.asarray(bs, np.uint64).view(np.int64).copy()).to(dev)


def as_u64(t):
    return t.detach().cpu().numpy().view(np.uint64)
