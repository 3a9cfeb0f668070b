"""The population evaluation and the cross-entropy tuner (evaluation/tune.py) on the host backend, no GPU involved.

* ``evaluate_population`` against ``evaluate_agent(HandPlanAgent(...))``, candidate by candidate: the games are seeded
  and the search is exact, so the scores are equal, not close.
* ``cem``: the same rng gives the same history; one generation against a numpy restatement (exact float64 equality,
  the same operations); a synthetic fitness with a known optimum direction improves.
* ``tune`` end to end, two generations: the log, candidate 0's fitness against ``evaluate_agent`` on the generation's
  seeds, and the written JSON loaded by ``HandPlanAgent.load``.
"""
import json
import math

import numpy as np
import pytest
import torch

FREE7 = [0, 1, 2, 3, 4, 5, 7]  # every weight but "dead" (index 6), as tune's default


@pytest.fixture(scope="module", autouse=True)
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


def test_evaluate_population_equals_one_agent_per_candidate():
    from agents.greedy import DEFAULT_WEIGHTS, HandPlanAgent
    from evaluation.evaluate import evaluate_agent
    from evaluation.tune import evaluate_population
    from runtime.lib import GREEDY_FIELDS

    sets = [{}, dict(DEFAULT_WEIGHTS), {"lines": 100}]
    seed, games, moves = 11, 3, 40
    got = evaluate_population(sets, games, moves, seed, depth=2, device="cpu")
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, games)
    for c, w in enumerate(sets):
        # a candidate's missing weights are 0 (weight_rows); a HandPlanAgent would fill them from its defaults
        full = {k: w.get(k, 0) for k in GREEDY_FIELDS}
        want = evaluate_agent(HandPlanAgent(full, depth=2, device="cpu"), num_episodes=games, seed=seed,
                              max_moves=moves)
        assert got[c].tolist() == want["scores"], (c, got[c].tolist(), want["scores"])
    assert len({tuple(r) for r in got.tolist()}) == 3, "the three candidates play the same: the test shows nothing"


def test_population_agent_with_default_rows_is_the_plan_agent():
    from agents.greedy import DEFAULT_WEIGHTS, HandPlanAgent, PopulationPlanAgent
    from evaluation.evaluate import evaluate_agent
    from runtime import kernels as K

    n = 5
    for depth, one in ((3, HandPlanAgent(device="cpu")), (0, HandPlanAgent(depth=1, device="cpu"))):
        pop = PopulationPlanAgent(K.weight_rows(DEFAULT_WEIGHTS, n=n), depth=depth, device="cpu")
        a = evaluate_agent(pop, num_episodes=n, seed=42, max_moves=30)
        b = evaluate_agent(one, num_episodes=n, seed=42, max_moves=30)
        assert a["scores"] == b["scores"] and a["lengths"] == b["lengths"], depth
    with pytest.raises(ValueError):
        PopulationPlanAgent(K.weight_rows({}, n=1), depth=4, device="cpu")


def test_evaluate_agent_seeds_default_is_seed_plus_episode():
    from agents.greedy import HandPlanAgent
    from evaluation.evaluate import evaluate_agent

    agent = HandPlanAgent(depth=1, device="cpu")
    a = evaluate_agent(agent, num_episodes=3, seed=7, max_moves=20)
    b = evaluate_agent(agent, num_episodes=3, seed=0, max_moves=20, seeds=[7, 8, 9])
    c = evaluate_agent(agent, num_episodes=3, seed=7, max_moves=20, seeds=[9, 9, 7])
    assert a["scores"] == b["scores"] and c["scores"] == [a["scores"][2], a["scores"][2], a["scores"][0]]
    with pytest.raises(ValueError):
        evaluate_agent(agent, num_episodes=3, seeds=[1, 2])


def _table_fitness(table):
    return lambda cand, k: np.asarray(table[k], dtype=np.float64)


def test_cem_is_deterministic_for_a_seed():
    from evaluation.tune import cem

    def fit(cand, k):
        return -np.abs(cand[:, FREE7].astype(np.float64) - 300.0).sum(axis=1)

    mean0 = [100, 0, -30, -2, 0, 1, -100000, 0]
    runs = [cem(fit, mean0, 300.0, 12, 0.25, 4, np.random.default_rng(5), FREE7) for _ in range(2)]
    other = cem(fit, mean0, 300.0, 12, 0.25, 4, np.random.default_rng(6), FREE7)
    for a, b in zip(*runs):
        for k in ("candidates", "fitness", "elite", "mean", "sigma"):
            assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(runs[0][0]["candidates"], other[0]["candidates"])
    for h in runs[0]:
        assert (h["candidates"][:, 6] == -100000).all(), "a fixed weight moved"
        assert (np.abs(h["candidates"][:, FREE7]).max(axis=1) == 1000).all(), "a candidate is off the scale"


def test_cem_one_generation_equals_numpy_restatement():
    from evaluation.tune import cem

    population, free, scale, floor = 8, [0, 2, 3], 1000.0, 10.0
    mean0 = np.array([50.0, 7.0, -20.0, 4.0])  # coordinate 1 is fixed
    sigma0 = np.array([30.0, 5.0, 0.5])
    table = [[3.0, 9.0, 1.0, 9.0, 2.0, 8.5, 9.0, 0.0]]  # a three-way tie for the best: the lower indices win
    h = cem(_table_fitness(table), mean0, sigma0, population, 0.3, 1, np.random.default_rng(123), free,
            scale=scale, sigma_floor=floor)[0]

    # the restatement: the same operations in the same order
    mean = mean0.copy()
    mean[free] = mean0[free] * (scale / np.max(np.abs(mean0[free])))
    z = np.random.default_rng(123).standard_normal((population - 1, len(free)))
    cand = np.tile(mean, (population, 1))
    cand[1:, free] = mean[free] + sigma0 * z
    top = np.max(np.abs(cand[:, free]), axis=-1, keepdims=True)
    cand[:, free] = cand[:, free] * (scale / top)
    cand = np.rint(cand).astype(np.int64)
    n_elite = math.ceil(population * 0.3)
    assert n_elite == 3
    elite = [1, 3, 6]
    want_mean = mean.copy()
    want_mean[free] = cand[elite][:, free].astype(np.float64).mean(axis=0)
    want_sigma = np.maximum(cand[elite][:, free].astype(np.float64).std(axis=0), floor)

    assert np.array_equal(h["candidates"], cand)
    assert h["candidates"][0].tolist() == [1000, 7, -400, 80]  # candidate 0: the mean itself, on the scale
    assert h["elite"].tolist() == elite
    assert np.array_equal(h["mean"], want_mean) and np.array_equal(h["sigma"], want_sigma)  # exact float64
    assert h["mean"][1] == 7.0 and (h["sigma"] >= floor).all()
    assert h["best_fitness"] == 9.0 and h["mean_fitness"] == float(np.mean(table[0]))


def test_cem_improves_a_synthetic_fitness():
    """Fitness = minus the distance from the candidate (already on the scale) to a target on the scale: the
    optimum is the target's direction.  The final mean must be nearer than the start."""
    from evaluation.tune import cem, normalise

    target = np.array([-200.0, 1000.0, 350.0, -700.0, 0.0, 90.0, 0.0, 500.0])

    def fit(cand, k=0):
        return -np.sqrt(((cand[:, FREE7].astype(np.float64) - target[FREE7]) ** 2).sum(axis=1))

    mean0 = np.array([100.0, 0, -30, -2, 0, 1, -100000, 0])
    hist = cem(fit, mean0, 300.0, 32, 0.25, 15, np.random.default_rng(2), FREE7)
    as_cand = lambda m: np.rint(normalise(m, FREE7, 1000))[None, :]  # noqa: E731
    first, last = fit(as_cand(mean0))[0], fit(as_cand(hist[-1]["mean"]))[0]
    print(f"synthetic fitness: start {first:.1f}, after 15 generations {last:.1f}")
    assert last > first
    assert hist[0]["fitness"][0] == first  # generation 0 plays the start mean as candidate 0


def test_tune_end_to_end_on_the_host_backend(tmp_path):
    from agents.greedy import HandPlanAgent
    from evaluation.evaluate import evaluate_agent
    from evaluation.tune import tune
    from runtime import lib as L

    # an init already on the scale (largest free weight 1000), so candidate 0 of generation 0 is init itself
    init = {"lines": 1000, "score": 0, "holes": -300, "filled": -20, "centre": 0, "mobility": 10, "dead": -100000,
            "refill": 0}
    out, log = tmp_path / "weights.json", tmp_path / "tune.jsonl"
    kw = dict(agent="plan", depth=2, population=6, games=2, moves=24, generations=2, seed=9, init=init, device="cpu",
              holdout_games=2)
    final = tune(output=str(out), log=str(log), **kw)
    records = [json.loads(ln) for ln in log.read_text().splitlines()]
    gens = [r for r in records if r["record"] == "generation"]
    assert len(gens) == 2 and [r["record"] for r in records] == ["generation", "generation", "final"]
    assert gens[0]["seeds"] == [9, 10] and gens[1]["seeds"] == [11, 12]  # fresh per generation, shared within it
    for r in gens:
        assert len(r["mean"]) == 8 and len(r["sigma"]) == 7 and r["mean"][6] == -100000
        assert r["best_fitness"] >= r["mean_fitness"]
    assert gens[0]["mean_played"] == init
    want = evaluate_agent(HandPlanAgent(init, depth=2, device="cpu"), num_episodes=2, max_moves=24, seeds=[9, 10])
    assert gens[0]["mean_played_fitness"] == float(np.mean(want["scores"]))
    last = records[-1]
    assert last["build_id"] == L.build_id(host=True) and last["holdout"]["seed0"] == 9 + 10 ** 6
    assert last["holdout"]["init"]["weights"] == init and last["holdout"]["tuned"]["weights"] == last["weights"]
    assert last["weights"] == final["weights"]

    doc = json.loads(out.read_text())
    assert doc == {"agent": "plan", "depth": 2, "weights": final["weights"]}
    agent = HandPlanAgent(depth=3, device="cpu")
    agent.load(str(out))
    assert agent.depth == 2 and agent.weights == final["weights"]

    again = tune(**kw)  # deterministic for a seed
    again.pop("wall_s"), final.pop("wall_s")
    assert again == final
