"""Shared by tests/test_safe_mask_host.py, tests/test_gpu_safe_mask.py and tests/test_gpu_safe_rollout.py: position
sets and references for the hand-safe mask call (bb_safe_mask), none of which calls it.

(a) the 92 positions of tests/_afterstates_ref.py with tests/_plan_values_ref.py's depth-2 "safe" / "legal";
(b) ``crowded``: 420 random boards at fill 0.35-0.9 (no full line) under random hands with every used pattern, which
    a random rollout never reaches; its reference is the host backend's bb_plan_values_pos at depth 2 (pinned by
    tests/test_plan_values_host.py): safe = its safe words, legal = q != INT64_MIN.
"""
import functools

import numpy as np
import torch

import _afterstates_ref as R
import _plan_values_ref as V


def crowded(n=420, seed=2024, fills=(0.35, 0.5, 0.6, 0.7, 0.8, 0.9), used=(0, 1, 2, 4, 3, 5, 6)):
    rng = np.random.default_rng(seed)
    boards = np.zeros(n, np.uint64)
    hands = np.zeros(n, np.uint32)
    for i in range(n):
        g = rng.random((8, 8)) < fills[i % 6]
        for r in range(8):
            if g[r].all():
                g[r, rng.integers(8)] = False
        for c in range(8):
            if g[:, c].all():
                g[rng.integers(8), c] = False
        boards[i] = sum(1 << (r * 8 + c) for r in range(8) for c in range(8) if g[r, c])
        ids = rng.integers(0, 37, 3)
        hands[i] = int(ids[0]) | int(ids[1]) << 6 | int(ids[2]) << 12 | used[(i // 6) % 7] << 18
    return boards, hands


def words(flags):
    """bool [n, 192] -> mask words u64 [n, 3] (bit c of word p = action p*64 + c)."""
    f = np.asarray(flags, bool).reshape(-1, 3, 64).astype(np.uint64)
    return (f << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def sampling(safe_words, legal_words):
    """Mode 1 from mode 0 and the legal words: where(any safe, safe, legal), row by row."""
    return np.where((safe_words != 0).any(axis=1, keepdims=True), safe_words, legal_words)


def host_safe_legal(board, hand):
    """(safe, legal) words u64 [n, 3] of bb_plan_values_pos at depth 2 on the host backend."""
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    out = K.plan_values(torch.from_numpy(np.asarray(board, np.uint64).view(np.int64).copy()),
                        torch.from_numpy(np.asarray(hand, np.uint32).view(np.int32).copy()), {}, 2, want=("q", "safe"))
    return out["safe"].numpy().view(np.uint64).copy(), words(out["q"].numpy() != R.INT64_MIN)


@functools.lru_cache(maxsize=None)
def reference_a():
    """Set (a): {"board", "hand", "safe", "legal", "mode1"}; safe / legal / mode1 are words u64 [92, 3]."""
    ref, want = R.reference(), V.reference_values(2)
    safe, legal = words(want["safe"]), words(want["legal"])
    assert int((want["legal"] & ~want["safe"]).sum()) >= 40
    assert bool(((legal != 0).any(axis=1) & (safe == 0).all(axis=1)).any())  # legal moves and none safe
    return {"board": ref["board"], "hand": ref["hand"], "safe": safe, "legal": legal, "mode1": sampling(safe, legal)}


@functools.lru_cache(maxsize=None)
def reference_b():
    """Set (b), the same keys, with the lower bounds on what it covers asserted on the reference side."""
    board, hand = crowded()
    safe, legal = host_safe_legal(board, hand)
    assert not (safe & ~legal).any()
    sb, lb = V.safe_bool(safe), V.safe_bool(legal)
    n_legal, n_safe = lb.sum(axis=1), sb.sum(axis=1)
    unsafe, none_safe = int((lb & ~sb).sum()), int(((n_legal > 0) & (n_safe == 0)).sum())
    proper = int(((n_safe > 0) & (n_safe < n_legal)).sum())
    print(f"crowded set: {int(lb.sum())} legal actions, {unsafe} unsafe, {none_safe} positions without a safe move, "
          f"{proper} with a proper non-empty safe subset")
    assert unsafe >= 200 and none_safe >= 20 and proper >= 30
    return {"board": board, "hand": hand, "safe": safe, "legal": legal, "mode1": sampling(safe, legal)}


def tensors(board, hand, dev):
    return (torch.from_numpy(np.asarray(board, np.uint64).view(np.int64).copy()).to(dev),
            torch.from_numpy(np.asarray(hand, np.uint32).view(np.int32).copy()).to(dev))


def as_u64(t):
    """A mask tensor int64 [n, 3] (any device) as numpy u64."""
    return t.detach().cpu().numpy().view(np.uint64).reshape(-1, 3)


def assert_words(got, want, what):
    got = as_u64(got) if isinstance(got, torch.Tensor) else got
    bad = np.argwhere((got != want).any(axis=1)).flatten()[:4]
    assert bad.size == 0, (what, bad.tolist(), [[hex(int(x)) for x in got[b]] for b in bad],
                           [[hex(int(x)) for x in want[b]] for b in bad])


def mid_hand_rule(hand, dones, mask, mode1_of_safe_legal):
    """The rollout property: every termination on a move that is not the hand's third traces back, within the same
    hand of the same env, to a step whose stored mask was the fallback.  hand i32 / dones [T, N], mask u64 [T, N, 3];
    mode1_of_safe_legal = (safe, legal) words [T, N, 3] of the stored positions.  Returns the number of mid-hand
    terminations."""
    safe, legal = mode1_of_safe_legal
    used = (np.asarray(hand).astype(np.int64) >> 18) & 7
    third = np.isin(used, (3, 5, 6))
    fallback = (safe == 0).all(axis=2) & (legal != 0).any(axis=2)
    T, N = used.shape
    count = 0
    for t, i in np.argwhere((np.asarray(dones) > 0) & ~third):
        count += 1
        s = t
        while s > 0 and used[s, i] != 0:
            s -= 1  # back to the first move of this hand (a reset or a refill leaves used == 0)
        if used[s, i] == 0:  # else the hand began before the stored rows: its first moves cannot be traced here
            assert fallback[s:t + 1, i].any(), ("mid-hand termination without a fallback step", int(t), int(i))
    return count
