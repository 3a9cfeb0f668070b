"""``evaluate_population(census=True)`` on the MI355X against the host backend: the same scores and the same extras
(P = 4, G = 3, 30 moves, depth 3).  The extras are computed on the host from the integer census counts
(``evaluation.evaluate.census_summary``), so they are equal, not merely close."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SETS = [{"lines": 100, "score": 0, "holes": -30, "filled": -2, "centre": 0, "mobility": 1, "dead": -100000, "refill": 0},
        {"lines": 10, "score": 3, "holes": 5, "filled": 4, "centre": 2, "mobility": -1, "dead": -100000, "refill": 0},
        {"lines": 0, "score": 1, "holes": 0, "filled": 6, "centre": 3, "mobility": 0, "dead": -100000, "refill": 0},
        {"lines": 1000, "score": 191, "holes": -374, "filled": -14, "centre": -19, "mobility": 12, "dead": -100000,
         "refill": 5}]


def test_population_census_equals_the_host_backend(cuda):
    from evaluation.tune import EXTRAS, evaluate_population
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    want_s, want_x = evaluate_population(SETS, 3, 30, 77, depth=3, device="cpu", census=True)
    got_s, got_x = evaluate_population(SETS, 3, 30, 77, depth=3, device=cuda, census=True)
    assert torch.equal(got_s, want_s)
    assert torch.equal(got_s, evaluate_population(SETS, 3, 30, 77, depth=3, device=cuda))
    for k in EXTRAS:
        assert torch.equal(got_x[k], want_x[k]), k
    assert (want_x["refills"] >= 1).all() and (want_x["min_solvable_fraction"] < 1).any()
