"""``PlayoutPlanAgent``, ``playout_scores`` and ``tune(engine="playout")`` on the host backend (CPU).

With ``hands=1`` the agent plays ``TwoHandShapeAgent``'s moves; with ``hands=2`` every decision equals steps 1-6
restated in numpy and plain Python over tests/_values_ext_ref.py and the playout oracle of tests/_playout_ref.py, which
call none of bb_plan_values_ext, bb_play_plan_pos or bb_playout_values; ``playout_scores`` is the same games played call
by call through the existing entry points; and the tuner's playout engine is deterministic under its seed."""
import json

import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _play_plan_ref as PP
import _playout_ref as PR
import _plan2_ref as P2
import _values_ext_ref as X

INT64_MIN = R.INT64_MIN


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.mark.parametrize("weights", [PR.SHAPED, dict(R.DEFAULT_WEIGHTS)], ids=["shaped", "eight"])
def test_one_hand_plays_the_two_hand_shape_agent_move_for_move(host, weights):
    from agents import PlayoutPlanAgent
    from agents.greedy import TwoHandShapeAgent

    seeds = [3, 5, 8, 13]
    kw = dict(depth=3, candidates=3, deals=3, seed=9, device="cpu")
    want = P2.play(TwoHandShapeAgent(weights, **kw), seeds, 12)
    got = P2.play(PlayoutPlanAgent(weights, hands=1, **kw), seeds, 12)
    assert got == want and len({tuple(m) for m in got}) > 6
    two = P2.play(PlayoutPlanAgent(weights, hands=2, **kw), seeds, 12)
    assert two != want  # the second hand changes decisions


def one_piece_left():
    """(board u64, hand u32): dense census boards with one piece left in the hand -- every move is a refill, so every
    candidate is valued by playouts, and the depth-3 trees behind them stay small."""
    import _census_ref as CR

    bs = CR.boards()
    board = np.array([int(bs[5]), int(bs[8]), int(bs[11])], np.uint64)
    hand = np.array([0 | 1 << 6 | 2 << 12 | 3 << 18, 5 | 0 << 6 | 7 << 12 | 5 << 18, 9 | 3 << 6 | 0 << 12 | 6 << 18],
                    np.uint32)  # slots used: 0 and 1; 0 and 2; 1 and 2
    return board, hand


def test_two_hands_against_steps_1_to_6_restated_over_the_reference(host):
    from agents import PlayoutPlanAgent

    w, k, deals, hands, seed = PR.SHAPED, 2, 2, 2, 77
    board, hand = one_piece_left()
    n = len(board)
    combo = np.zeros(n, np.int32)
    per = X.per_action_ext(board, hand, combo, 3, {"w": w})                 # step 1
    q, rest = per["q"]["w"], per["rest"]["w"]
    key = (seed + 0x9E3779B97F4A7C15) % 2 ** 64                             # the deals of decision 0
    rows = []
    for i in range(n):
        order = np.argsort(-q[i].astype(object), kind="stable")             # step 2
        for a in [int(a) for a in order if q[i, a] != INT64_MIN][:k]:
            a2, a3 = int(rest[i, a]) & 0xFF, (int(rest[i, a]) >> 8) & 0xFF
            env = R.make_env(int(board[i]), [(int(hand[i]) >> (6 * s)) & 63 for s in range(3)],
                             used=[bool((int(hand[i]) >> (18 + s)) & 1) for s in range(3)])
            rows.append((i, a, PP.oracle_play(env, [a, -1 if a2 == 0xFF else a2, -1 if a3 == 0xFF else a3])))  # step 3
    assert len(rows) >= n + 2 and all(leaf[5] & PP.REFILL for _, _, leaf in rows)  # a choice to make at two boards
    ref = PR.oracle(np.array([leaf[0] for _, _, leaf in rows], np.uint64), w, 3, deals, hands, key,   # step 4
                    combo=[leaf[2] for _, _, leaf in rows], stream=[i for i, _, _ in rows])
    one, two = ref[1]["value"], ref[2]["value"]
    assert (one != two).any() and (ref[2]["hands"] == 2).all()               # the second hand is in the values
    q2 = {}
    for (i, a, leaf), values in zip(rows, two):
        q2[i, a] = deals * (w["lines"] * leaf[3] + w["score"] * leaf[4]) + int(values.sum())
    want = [-max((v, -a) for (e, a), v in q2.items() if e == i)[1] for i in range(n)]   # step 6
    agent = PlayoutPlanAgent(w, depth=3, candidates=k, deals=deals, hands=hands, seed=seed, device="cpu")
    tb, th = PR.board_tensor(board), torch.from_numpy(hand.view(np.int32).copy())
    pv = agent._plan_values_pos(tb, th)
    got = agent._decide(tb, th, torch.zeros(n, dtype=torch.int32), pv["q"], pv["rest"])
    assert got.tolist() == want and agent.moves == 1


def test_save_load_carry_the_hands_and_the_command_lines_choose_the_class(host, tmp_path, monkeypatch):
    import evaluation.evaluate as EV
    import evaluation.tune as T
    from agents import PlayoutPlanAgent
    from agents.greedy import DEFAULT_WEIGHTS, TwoHandShapeAgent

    a = PlayoutPlanAgent(PR.SHAPED, depth=2, candidates=5, deals=9, hands=7, seed=4, device="cpu")
    path = str(tmp_path / "a.json")
    a.save(path)
    data = json.load(open(path))
    assert data["agent"] == "playout" and data["hands"] == 7 and data["weights"] == {**DEFAULT_WEIGHTS, **PR.SHAPED}
    b = PlayoutPlanAgent(device="cpu")
    assert b.hands == 2  # the untuned default
    b.load(path)
    assert (b.depth, b.candidates, b.deals, b.hands, b.seed, b.weights) == (2, 5, 9, 7, 4, a.weights)
    c = TwoHandShapeAgent(device="cpu")
    c.load(path)  # the parent reads the same file and ignores the hands
    assert (c.candidates, c.deals) == (5, 9)
    for hands in (0, 257):
        with pytest.raises(ValueError, match="hands must be 1..256"):
            PlayoutPlanAgent(hands=hands, device="cpu")
    # evaluate.py --agent playout --hands H
    evaluate_agent = EV.evaluate_agent
    built = []
    monkeypatch.setattr(EV, "evaluate_agent", lambda agent, **kw: built.append(agent) or {})
    monkeypatch.setattr(EV, "print_results", lambda res: None)
    monkeypatch.setattr("sys.argv", ["evaluate.py", "--agent", "playout", "--device", "cpu", "--candidates", "3",
                                     "--deals", "2", "--hands", "3", "--weights", path])
    EV.main()
    assert type(built[0]) is PlayoutPlanAgent
    assert (built[0].depth, built[0].candidates, built[0].deals, built[0].hands) == (3, 3, 2, 3)
    # tune.py --compare FILE --agent playout --hands H: compare_two_hand's records, the agent class chosen there
    recs = T.compare_two_hand([dict(DEFAULT_WEIGHTS), PR.SHAPED], 2, 9, 5, depth=3, candidates=2, deals=2, device="cpu",
                              hands=2)
    for w, rec in zip((dict(DEFAULT_WEIGHTS), PR.SHAPED), recs):
        agent = PlayoutPlanAgent(w, depth=3, candidates=2, deals=2, hands=2, seed=5, device="cpu")
        one = evaluate_agent(agent, num_episodes=2, seeds=[5, 6], max_moves=9)
        assert rec["mean_score"] == pytest.approx(float(np.mean(one["scores"])))
    seen = {}
    monkeypatch.setattr(T, "compare_two_hand", lambda *a, **kw: seen.update(kw) or [{}, {}])
    monkeypatch.setattr("sys.argv", ["tune.py", "--compare", path, "--agent", "playout", "--hands", "3", "--device",
                                     "cpu", "--games", "2"])
    T.main()
    assert seen == {"hands": 3}


def test_playout_scores_are_the_games_played_call_by_call(host):
    from evaluation.tune import playout_scores

    sets = [PR.SHAPED, PR.PLAIN, PR.ANTI, PR.SCORED]
    rows = PR.rows_of(sets)
    games, hands, seed = 3, 5, 21
    score, plies, status = playout_scores(rows, games, hands, seed, device="cpu")
    zeros = torch.zeros(len(sets), dtype=torch.int64)
    want = PR.composed(zeros, rows, 3, games, hands, seed, stream=zeros)
    assert torch.equal(score, want["score"]) and torch.equal(plies, want["plies"]) and torch.equal(status, want["status"])
    assert tuple(score.shape) == (4, 3) and (plies == 3 * hands).any() and (score > 0).all()
    # stream id 0 for every board: all candidates are dealt the same first hand of a game
    first = PR.call(zeros, rows, 3, games, 1, seed, stream=zeros, want=("hand",))["hand"]
    assert (first == first[0]).all() and len(set(first[0].tolist())) > 1


def test_tune_with_the_playout_engine(host, tmp_path, monkeypatch):
    import evaluation.tune as T

    calls = []
    real = T.playout_scores
    monkeypatch.setattr(T, "playout_scores", lambda *a, **k: calls.append(a[1:4]) or real(*a, **k))
    log = str(tmp_path / "log.jsonl")
    kw = dict(agent="plan", depth=3, population=4, games=2, moves=7, generations=2, seed=5, device="cpu",
              holdout_games=2, engine="playout", terms=("room5",))
    final = T.tune(log=log, **kw)
    assert final["settings"]["engine"] == "playout" and final["settings"]["hands"] == 3  # ceil(7 / 3)
    assert [c[:2] for c in calls] == [(2, 3), (2, 3)] and calls[0][2] != calls[1][2]  # a key of its own per generation
    again = T.tune(**kw)
    assert again["weights"] == final["weights"] and again["holdout"] == final["holdout"]
    gen = [json.loads(line) for line in open(log)][0]
    from agents.greedy import TwoHandPlanAgent

    score, _, _ = real(PR.rows_of(gen["mean_played"]), 2, 3, TwoHandPlanAgent.deal_seed(5, 0), 3, "cpu")
    assert gen["mean_played_fitness"] == float(score.double().mean())
    with pytest.raises(ValueError, match=r"hands must be 1\.\.256"):
        T.tune(**{**kw, "moves": 769})
    with pytest.raises(ValueError, match="engine 'playout' plays the plan agent"):
        T.tune(**{**kw, "agent": "plan2"})
    with pytest.raises(ValueError, match="engine must be"):
        T.tune(**{**kw, "engine": "dice"})
    # the default engine is untouched: no playout call, the settings it had
    del calls[:]
    plain = T.tune(**{k: v for k, v in kw.items() if k != "engine"})
    assert not calls and "engine" not in plain["settings"] and "hands" not in plain["settings"]
    seen = {}
    monkeypatch.setattr(T, "tune", lambda **kw: seen.update(kw) or {"record": "final"})
    monkeypatch.setattr("sys.argv", ["tune.py", "--engine", "playout", "--device", "cpu"])
    T.main()
    assert seen["engine"] == "playout" and seen["agent"] == "plan"
