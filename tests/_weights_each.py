"""Shared by tests/test_weights_each_host.py and tests/test_gpu_weights_each.py: the four weight sets, how they are
dealt over positions, and the gather that turns four uniform calls into the expectation of one per-position call."""
import numpy as np
import torch

import _afterstates_ref as R

CPU = torch.device("cpu")
BIG = 2 ** 31 - 1
# {}, the defaults, the defaults with every sign turned, and weights at the ends of int32
SETS = [{}, dict(R.DEFAULT_WEIGHTS), {k: -v for k, v in R.DEFAULT_WEIGHTS.items()},
        {"lines": BIG, "score": -BIG, "holes": -BIG, "filled": BIG, "centre": -BIG, "mobility": BIG, "dead": -BIG,
         "refill": BIG}]
KEYS = ("action", "value", "plan", "leaves")


def mixed_rows(n, dev=CPU, shift=0):
    """(rows int32 [n, 8], set index [n]): position i takes SETS[(i + shift) % 4]."""
    from runtime import kernels as K

    which = (np.arange(n) + shift) % len(SETS)
    return K.weight_rows([SETS[j] for j in which], device=dev), which


def gathered(uniform_results, which):
    """Row i of the uniform call made under the set position i was dealt."""
    sel = torch.as_tensor(which)
    return {k: torch.stack([r[k] for r in uniform_results])[sel, torch.arange(len(which))]
            for k in uniform_results[0]}


def no_action_positions(ref):
    """A finished game (the crafted "game_over") and its board with a hand that is not flagged over but fits
    nowhere (two DOMINO_H and a SQUARE_3x3 on the board whose free cells are never adjacent), each four times."""
    i = ref["names"]["game_over"]
    stuck = 1 | (1 << 6) | (36 << 12)
    board = torch.from_numpy(np.array([ref["board"][i]] * 8, np.uint64).view(np.int64))
    hand = torch.tensor([int(ref["hand"][i])] * 4 + [stuck] * 4, dtype=torch.int32)
    return board, hand
