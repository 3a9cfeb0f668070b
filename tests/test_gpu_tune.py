"""``evaluate_population`` (evaluation/tune.py) on the MI355X against the host backend: P = 4 candidates, G = 3
shared piece streams, 30 moves, depth 3.  The env and the search are bit-exact across the backends
(tests/test_gpu_env_parity.py, tests/test_gpu_weights_each.py), so the [P, G] scores are equal, not close."""
import pytest
import torch

from _weights_each import SETS

pytestmark = pytest.mark.gpu


def test_evaluate_population_equals_host_backend(cuda):
    from evaluation.tune import evaluate_population
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    sets = [SETS[1], SETS[0], {"lines": 100}, SETS[2]]  # defaults, zeros, lines only, the defaults turned round
    got = evaluate_population(sets, games=3, moves=30, seed=21, depth=3, device=cuda)
    want = evaluate_population(sets, games=3, moves=30, seed=21, depth=3, device="cpu")
    assert got.dtype == torch.int64 and tuple(got.shape) == (4, 3)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert len({tuple(r) for r in want.tolist()}) > 1, "every candidate scored the same: the test shows nothing"
    greedy = evaluate_population(sets, games=3, moves=30, seed=21, depth=0, device=cuda)  # the one-ply kernel
    assert torch.equal(greedy, evaluate_population(sets, games=3, moves=30, seed=21, depth=1, device="cpu"))
