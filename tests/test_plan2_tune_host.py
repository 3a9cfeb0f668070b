"""The tuner on the two-hand agent (``tune(agent="plan2")``, ``tune.py --agent plan2``) on the host backend (CPU): the
population played by ``PopulationTwoHandAgent`` scores, row by row, what the single-set two-hand agents score on the
same seeds; the held-out comparison is ``compare_two_hand``'s; the output is a file ``TwoHandPlanAgent.load`` reads; and
with agent "plan" nothing of this is touched."""
import json

import numpy as np
import pytest
import torch

import _plan2_ref as P2


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


SETS = [dict(P2.R.DEFAULT_WEIGHTS), P2.SHAPED, {**P2.R.DEFAULT_WEIGHTS, "holes": -5, "lines": 300, "room5": 7}]


def test_row_c_of_the_population_is_the_single_set_agent(host):
    """A 3 x 2 population of 6 moves, depth 2."""
    from agents.greedy import two_hand_agent_class
    from evaluation.evaluate import evaluate_agent
    from evaluation.tune import evaluate_population

    kw = dict(candidates=3, deals=2)
    scores = evaluate_population(SETS, 2, 6, 31, 2, "cpu", two_hand=kw)
    assert tuple(scores.shape) == (3, 2)
    for c, w in enumerate(SETS):
        agent = two_hand_agent_class(w)(w, depth=2, seed=31, device="cpu", **kw)
        one = evaluate_agent(agent, num_episodes=2, seeds=[31, 32], max_moves=6)
        assert scores[c].tolist() == [int(x) for x in one["scores"]], c
    plain = evaluate_population(SETS, 2, 6, 31, 2, "cpu")
    assert tuple(plain.shape) == (3, 2)


def test_tune_plan2_runs_writes_a_loadable_file_and_compares_like_compare_two_hand(host, tmp_path):
    from agents.greedy import TwoHandShapeAgent
    from evaluation.tune import HOLDOUT_SEED_OFFSET, compare_two_hand, tune

    out, log = str(tmp_path / "w.json"), str(tmp_path / "log.jsonl")
    kw = dict(agent="plan2", depth=2, population=3, games=2, moves=6, generations=2, seed=5, device="cpu",
              holdout_games=2, candidates=3, deals=2, terms=("room5",))
    final = tune(output=out, log=log, **kw)
    assert final["agent"] == "plan2" and final["depth"] == 2
    assert final["settings"]["candidates"] == 3 and final["settings"]["deals"] == 2
    assert final["settings"]["terms"] == ["room5"] and "room5" in final["weights"]
    doc = json.load(open(out))
    assert set(doc) == {"agent", "depth", "candidates", "deals", "seed", "weights"} and doc["agent"] == "plan2"
    agent = TwoHandShapeAgent(device="cpu")
    agent.load(out)
    assert (agent.depth, agent.candidates, agent.deals, agent.seed) == (2, 3, 2, 5)
    # the eight-weight agent refuses a shape weight's name even at 0: compare_two_hand gets the sets without those
    sets = [{k: v for k, v in w.items() if v or k in P2.R.DEFAULT_WEIGHTS} for w in (final["init"], final["weights"])]
    held = compare_two_hand(sets, 2, 6, 5 + HOLDOUT_SEED_OFFSET, depth=2, candidates=3, deals=2, device="cpu")
    for mine, theirs in zip((final["holdout"]["init"], final["holdout"]["tuned"]), held):
        assert {k: v for k, v in mine.items() if k != "weights"} == {k: v for k, v in theirs.items() if k != "weights"}
    again = tune(**kw)
    assert again["weights"] == final["weights"] and again["holdout"] == final["holdout"]
    records = [json.loads(line) for line in open(log)]
    assert [r["record"] for r in records] == ["generation", "generation", "final"]
    assert records[1]["seeds"] == [5 + 2, 5 + 3]
    with pytest.raises(ValueError, match="candidates must be"):
        tune(**{**kw, "candidates": 0})
    with pytest.raises(ValueError, match="terms need agent"):
        tune(**{**kw, "agent": "greedy"})


def test_tune_plan_makes_no_two_hand_call_and_its_records_stand(host, tmp_path, monkeypatch):
    """agent "plan": no ``PopulationTwoHandAgent`` is built, the record is reproducible for a fixed seed, candidate 0's
    fitness is ``evaluate_population``'s of the mean as played, and the file has the three keys it had."""
    import evaluation.tune as T

    built = []
    real = T.PopulationTwoHandAgent
    monkeypatch.setattr(T, "PopulationTwoHandAgent", lambda *a, **k: built.append(1) or real(*a, **k))
    out, log = str(tmp_path / "w.json"), str(tmp_path / "log.jsonl")
    kw = dict(agent="plan", depth=2, population=3, games=2, moves=6, generations=2, seed=5, device="cpu",
              holdout_games=2)
    final = T.tune(output=out, log=log, **kw)
    assert not built and T.tune(**kw)["weights"] == final["weights"]
    assert set(json.load(open(out))) == {"agent", "depth", "weights"}
    assert set(final["settings"]) == {"population", "games", "moves", "generations", "elite_frac", "seed", "sigma0",
                                      "scale", "sigma_floor"}
    gen = [json.loads(line) for line in open(log)][0]
    played = T.evaluate_population([gen["mean_played"]], 2, 6, 5, 2, "cpu")
    assert gen["mean_played_fitness"] == float(played.double().mean())
    rng = np.random.default_rng(5)  # the draws are those of cem alone: one standard_normal((P - 1, free)) a generation
    assert rng.standard_normal((2, 7)).shape == (2, 7) and len(gen["sigma"]) == 7


def test_the_command_line_accepts_plan2_without_compare(host, monkeypatch, capsys):
    import evaluation.tune as T

    seen = {}
    monkeypatch.setattr(T, "tune", lambda **kw: seen.update(kw) or {"record": "final"})
    monkeypatch.setattr("sys.argv", ["tune.py", "--agent", "plan2", "--candidates", "4", "--deals", "6", "--depth", "2",
                                     "--terms", "room5,fits", "--device", "cpu"])
    T.main()
    assert seen["agent"] == "plan2" and seen["candidates"] == 4 and seen["deals"] == 6
    assert seen["terms"] == ["room5", "fits"] and json.loads(capsys.readouterr().out) == {"record": "final"}
    seen.clear()
    monkeypatch.setattr("sys.argv", ["tune.py", "--agent", "plan", "--device", "cpu"])
    T.main()
    assert "candidates" not in seen and "deals" not in seen
