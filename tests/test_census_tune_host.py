"""The refill census in the evaluator and the tuner, on the host backend (no GPU involved):

* ``evaluate_population(census=True)``: the scores are those of the call without the census, and the extras equal a
  restatement that replays every game on an env of its own, move by move, and asks tests/_census_ref.py's oracle
  census at each refill (hazards as exact fractions);
* ``evaluate_agent(census=False)`` and ``tune(fitness="score")`` keep exactly their keys;
* ``tune(fitness="survival")`` end to end: candidate 0's logged fitness is the formula on an independent
  ``evaluate_population(census=True)`` call, and a second run is identical.
"""
import fractions
import json

import numpy as np
import pytest
import torch

import _census_ref as CR

SETS = [{"lines": 100, "score": 0, "holes": -30, "filled": -2, "centre": 0, "mobility": 1, "dead": -100000, "refill": 0},
        {"lines": 10, "score": 3, "holes": 5, "filled": 4, "centre": 2, "mobility": -1, "dead": -100000, "refill": 0}]
GAMES, MOVES, SEED, DEPTH = 2, 30, 21, 2


@pytest.fixture(scope="module", autouse=True)
def host():
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)


def _replay(weights, seed):
    """One game on an env of its own: (score, length, [census count of the board after each refill])."""
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(1, [seed], autoreset=False, device="cpu")
    env.reset()
    act = torch.zeros(1, dtype=torch.int32)
    counts, length = [], 0
    for _ in range(MOVES):
        env.plan_actions(act, weights, depth=DEPTH)
        env.step(act)
        length += 1
        st = env.state()
        if bool(env.terminated[0]):
            break
        if (int(st["hand"][0]) >> 18) & 7 == 0:  # a whole hand after a move: the dealer has just run
            counts.append(int(CR.oracle_census(st["board"])[0][0]))
    score = int(env.state()["score"][0])
    env.close()
    return score, length, counts


def _close(got, want):
    return abs(got - want) <= 1e-12 * abs(want)


def test_population_extras_equal_a_replay_through_the_oracle():
    from evaluation.tune import EXTRAS, evaluate_population

    plain = evaluate_population(SETS, GAMES, MOVES, SEED, depth=DEPTH, device="cpu")
    scores, extras = evaluate_population(SETS, GAMES, MOVES, SEED, depth=DEPTH, device="cpu", census=True)
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, scores)
    assert set(extras) == set(EXTRAS)
    for k in EXTRAS:
        assert extras[k].shape == (2, GAMES) and extras[k].dtype == (torch.int64 if k == "refills" else torch.float64)
    some_risk = False
    for c, w in enumerate(SETS):
        for g in range(GAMES):
            score, length, counts = _replay(w, SEED + g)
            assert score == int(scores[c, g])
            hz = [fractions.Fraction(CR.NUM_HANDS - k, CR.NUM_HANDS) ** 100 for k in counts]
            assert int(extras["refills"][c, g]) == len(counts) and len(counts) >= 1
            assert _close(float(extras["expected_losses"][c, g]), float(sum(hz))), (c, g)
            assert _close(float(extras["survival"][c, g]), float(np.prod([1 - h for h in hz]))), (c, g)
            assert float(extras["min_solvable_fraction"][c, g]) == min(counts) / CR.NUM_HANDS
            some_risk |= min(counts) < CR.NUM_HANDS
    assert some_risk  # not every board of these games takes every hand


def test_evaluate_agent_keeps_its_keys_without_the_census():
    from agents.greedy import HandPlanAgent
    from evaluation.evaluate import CENSUS_KEYS, evaluate_agent

    agent = HandPlanAgent(SETS[0], depth=DEPTH, device="cpu")
    base = {"num_episodes", "mean_score", "std_score", "min_score", "max_score", "median_score", "mean_length",
            "std_length", "mean_lines_cleared", "mean_max_combo", "scores", "lengths"}
    plain = evaluate_agent(agent, num_episodes=2, seed=SEED, max_moves=MOVES)
    off = evaluate_agent(agent, num_episodes=2, seed=SEED, max_moves=MOVES, census=False)
    on = evaluate_agent(agent, num_episodes=2, seed=SEED, max_moves=MOVES, census=True)
    assert set(plain) == set(off) == base and plain == off
    assert set(on) == base | set(CENSUS_KEYS) | {f"mean_{k}" for k in CENSUS_KEYS}
    assert {k: on[k] for k in base} == plain
    for k in CENSUS_KEYS:
        assert len(on[k]) == 2 and on[f"mean_{k}"] == pytest.approx(np.mean(on[k]), rel=1e-15)
    assert on["refills"] == [MOVES // 3] * 2


TUNE = dict(agent="plan", depth=DEPTH, population=4, games=2, moves=12, generations=2, seed=3, device="cpu",
            holdout_games=2)
GEN_KEYS = {"record", "generation", "seeds", "best_fitness", "mean_fitness", "mean_played", "mean_played_fitness",
            "best", "mean", "sigma"}
FINAL_KEYS = {"record", "agent", "depth", "weights", "init", "fixed", "holdout", "settings", "build_id", "backend",
              "wall_s"}
HELD_KEYS = {"weights", "mean_score", "mean_length", "ended_before_cut", "score_per_move", "score_per_move_se"}


def _records(path):
    return [json.loads(ln) for ln in path.read_text().splitlines()]


def test_tune_on_the_score_writes_the_records_it_wrote(tmp_path):
    from evaluation.tune import tune

    tune(**TUNE, log=str(tmp_path / "a.jsonl"))
    tune(**TUNE, fitness="score", log=str(tmp_path / "b.jsonl"))
    a, b = _records(tmp_path / "a.jsonl"), _records(tmp_path / "b.jsonl")
    for recs in (a, b):
        assert [set(r) for r in recs] == [GEN_KEYS, GEN_KEYS, FINAL_KEYS]
        assert set(recs[-1]["holdout"]["init"]) == set(recs[-1]["holdout"]["tuned"]) == HELD_KEYS
    for ra, rb in zip(a, b):
        assert {k: v for k, v in ra.items() if k != "wall_s"} == {k: v for k, v in rb.items() if k != "wall_s"}
    with pytest.raises(ValueError, match="fitness must be"):
        tune(**TUNE, fitness="hazard")


def test_tune_on_survival_end_to_end(tmp_path):
    from evaluation.tune import EXTRAS, evaluate_population, survival_fitness, tune

    out = []
    for name in ("a", "b"):
        final = tune(**TUNE, fitness="survival", log=str(tmp_path / f"{name}.jsonl"),
                     output=str(tmp_path / f"{name}.json"))
        assert final["fitness"] == "survival" and final["horizon"] == TUNE["moves"]
        out.append([{k: v for k, v in r.items() if k != "wall_s"} for r in _records(tmp_path / f"{name}.jsonl")])
    assert out[0] == out[1]
    assert (tmp_path / "a.json").read_text() == (tmp_path / "b.json").read_text()
    gens = out[0][:2]
    for r in gens:
        assert set(r) == GEN_KEYS | {"mean_played_extras", "best_extras"}
        assert set(r["mean_played_extras"]) == set(r["best_extras"]) == set(EXTRAS)
    assert set(out[0][-1]["holdout"]["tuned"]) == HELD_KEYS | set(EXTRAS)
    # candidate 0 of each generation, played again on its own
    for r in gens:
        seed0 = r["seeds"][0]
        assert r["seeds"] == [TUNE["seed"] + r["generation"] * 2 + g for g in range(2)]
        scores, extras = evaluate_population([r["mean_played"]], 2, TUNE["moves"], seed0, depth=DEPTH, device="cpu",
                                             census=True)
        lengths = torch.full_like(scores, TUNE["moves"])  # depth-2 play does not die within 12 moves
        want = float(survival_fitness(scores, lengths, extras["survival"], TUNE["moves"])[0])
        by_hand = np.mean([float(scores[0, g]) * float(extras["survival"][0, g]) ** (12 / 12) for g in range(2)])
        assert r["mean_played_fitness"] == want == by_hand
        assert r["mean_played_extras"] == {k: float(extras[k].double().mean()) for k in EXTRAS}


def test_survival_fitness_is_the_formula():
    from evaluation.tune import survival_fitness

    scores = torch.tensor([[100, 200, 50]])
    lengths = torch.tensor([[300, 150, 0]])
    surv = torch.tensor([[0.9, 0.5, 0.25]], dtype=torch.float64)
    want = np.mean([100 * 0.9 ** (300 / 300), 200 * 0.5 ** (300 / 150), 50 * 0.25 ** (300 / 1)])
    assert float(survival_fitness(scores, lengths, surv, 300)[0]) == pytest.approx(want, rel=1e-15)
