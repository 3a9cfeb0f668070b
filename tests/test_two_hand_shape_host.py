"""``TwoHandShapeAgent`` on the host backend (CPU), the command lines that choose it and the trainers' labelling.

With the four shape weights 0 the agent plays ``TwoHandPlanAgent``'s moves through the very same calls; with one
candidate it plays ``HandPlanAgent``'s moves under the same twelve weights; and with four candidates and four deals
every action equals a numpy restatement of steps 2-6 on the values of tests/_values_ext_ref.py, which calls none of
bb_plan_values_ext, bb_refill_values_ext or bb_play_plan_pos.
"""
import json

import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _play_plan_ref as PP
import _values_ext_ref as X

INT64_MIN = R.INT64_MIN
SHAPED = X.SETS["all"]
ZEROS = {k: 0 for k in ("perimeter", "room3", "room5", "fits")}


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


def _games(seeds):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(len(seeds), list(seeds), autoreset=False, device="cpu")
    env.reset()
    return env


def _play(agent, seeds, moves):
    env = _games(seeds)
    act = torch.zeros(len(seeds), dtype=torch.int32)
    log = []
    for _ in range(moves):
        agent.act_env(env, act)
        log.append(act.tolist())
        env.step(act)
    env.close()
    return log


def _calls(monkeypatch):
    """Record which runtime.kernels / DeviceEnvBatch search calls are made."""
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    seen = []
    for owner, names in ((K, ("plan_values", "plan_values_ext", "refill_values", "refill_values_ext")),
                         (DeviceEnvBatch, ("plan_values", "plan_values_ext"))):
        for name in names:
            real = getattr(owner, name)

            def spy(*a, _real=real, _tag=f"{owner.__name__.split('.')[-1]}.{name}", **kw):
                seen.append(_tag)
                return _real(*a, **kw)

            monkeypatch.setattr(owner, name, spy)
    return seen


def test_zero_shape_weights_play_the_two_hand_plan_agent_through_its_calls(host, monkeypatch):
    from agents.greedy import TwoHandPlanAgent, TwoHandShapeAgent

    seeds = [3, 5, 8, 13]
    kw = dict(depth=2, candidates=3, deals=2, seed=9, device="cpu")
    seen = _calls(monkeypatch)
    want = _play(TwoHandPlanAgent({"holes": -40}, **kw), seeds, 14)
    parent_calls = sorted(set(seen))
    del seen[:]
    got = _play(TwoHandShapeAgent({"holes": -40, **ZEROS}, **kw), seeds, 14)
    assert got == want and len({tuple(m) for m in got}) > 6
    assert sorted(set(seen)) == parent_calls == ["DeviceEnvBatch.plan_values", "kernels.refill_values"]
    del seen[:]
    shaped = _play(TwoHandShapeAgent({"holes": -40, **SHAPED}, **kw), seeds, 14)
    assert sorted(set(seen)) == ["DeviceEnvBatch.plan_values_ext", "kernels.refill_values_ext"]
    assert shaped != want


def test_one_candidate_plays_the_hand_plan_agent_under_the_twelve_weights(host):
    from agents.greedy import HandPlanAgent, TwoHandShapeAgent

    seeds = [3, 5, 8, 13]
    one = _play(TwoHandShapeAgent(SHAPED, depth=2, candidates=1, deals=3, seed=9, device="cpu"), seeds, 24)
    plan = _play(HandPlanAgent(SHAPED, depth=2, device="cpu"), seeds, 24)
    assert one == plan and one != _play(HandPlanAgent(depth=2, device="cpu"), seeds, 24)


def restated_actions(state, weights, depth, candidates, deals, seed, move):
    """Steps 1-6 of ``TwoHandShapeAgent`` for the envs of ``state`` (DeviceEnvBatch.state()): q and rest from the
    reference, steps 2-6 in plain Python and numpy."""
    board, hand, combo = state["board"], state["hand"], state["combo"]
    n = len(board)
    per = X.per_action_ext(board, hand, combo, depth, {"w": weights})   # step 1
    q, rest = per["q"]["w"], per["rest"]["w"]
    key = (int(seed) + (move + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
    rows = []  # (env, action, leaf) of every candidate
    for i in range(n):
        order = np.argsort(-q[i].astype(object), kind="stable")        # step 2: descending, ties to the lower action
        for a in [int(a) for a in order if q[i, a] != INT64_MIN][:candidates]:
            a2, a3 = int(rest[i, a]) & 0xFF, (int(rest[i, a]) >> 8) & 0xFF
            env = R.make_env(int(board[i]), [(int(hand[i]) >> (6 * s)) & 63 for s in range(3)],
                             used=[bool((int(hand[i]) >> (18 + s)) & 1) for s in range(3)], combo=int(combo[i]))
            rows.append((i, a, PP.oracle_play(env, [a, -1 if a2 == 0xFF else a2, -1 if a3 == 0xFF else a3])))  # step 3
    q2 = {}
    refills = [(i, a, leaf) for i, a, leaf in rows if leaf[5] & PP.REFILL]
    if refills:                                                         # step 4
        ref = X.refill_values_ext(np.array([leaf[0] for _, _, leaf in refills], np.uint64), deals, key, depth,
                                  {"w": weights}, combo=[leaf[2] for _, _, leaf in refills],
                                  stream=[i for i, _, _ in refills])
        for (i, a, leaf), values in zip(refills, ref["value"]["w"]):
            moved = weights["lines"] * leaf[3] + weights["score"] * leaf[4]
            q2[i, a] = deals * moved + int(values.sum())
    for i, a, leaf in rows:                                             # step 5
        q2.setdefault((i, a), deals * int(q[i, a]))
    actions = []
    for i in range(n):                                                  # step 6
        mine = [(v, -a) for (e, a), v in q2.items() if e == i]
        actions.append(-max(mine)[1] if mine else 0)
    return actions, len(refills), len(rows) - len(refills)


def test_four_candidates_four_deals_against_the_restatement(host):
    """8 positions (4 games x 2 decisions, the games moved on by the agent), depth 2."""
    from agents.greedy import DEFAULT_WEIGHTS, TwoHandShapeAgent

    weights = {**DEFAULT_WEIGHTS, **SHAPED}
    agent = TwoHandShapeAgent(SHAPED, depth=2, candidates=4, deals=4, seed=77, device="cpu")
    assert agent.weights == weights
    seeds = [21, 34, 55, 89]
    env = _games(seeds)
    act = torch.zeros(4, dtype=torch.int32)
    for _ in range(9):  # into the game: the boards are no longer empty
        agent.act_env(env, act)
        env.step(act)
    refills = others = differs = 0
    for move in range(9, 11):
        want, r, o = restated_actions(env.state(), weights, 2, 4, 4, 77, move)
        plain = torch.zeros(4, dtype=torch.int32)
        env.plan_actions_ext(plain, agent._ext_rows(torch.device("cpu")), 2)
        agent.act_env(env, act)
        assert act.tolist() == want, move
        refills, others, differs = refills + r, others + o, differs + int((plain != act).sum())
        env.step(act)
    env.close()
    assert agent.moves == 11 and refills >= 4 and others >= 4


def test_save_load_round_trip_and_the_refusals_that_stay(host, tmp_path):
    from agents.greedy import DEFAULT_WEIGHTS, GreedyAgent, TwoHandPlanAgent, TwoHandShapeAgent

    a = TwoHandShapeAgent(SHAPED, depth=2, candidates=5, deals=9, seed=4, device="cpu")
    path = str(tmp_path / "a.json")
    a.save(path)
    data = json.load(open(path))
    assert data["agent"] == "plan2" and data["weights"] == {**DEFAULT_WEIGHTS, **SHAPED} and len(data["weights"]) == 12
    b = TwoHandShapeAgent(device="cpu")
    b.load(path)
    assert (b.depth, b.candidates, b.deals, b.seed, b.weights) == (2, 5, 9, 4, a.weights)
    assert _play(a, [7, 8], 6) == _play(b, [7, 8], 6)
    with pytest.raises(ValueError, match="unknown evaluation weights"):
        TwoHandShapeAgent({"room4": 1}, device="cpu")
    for cls in (GreedyAgent, TwoHandPlanAgent):  # the eight-weight agents keep their refusal
        with pytest.raises(ValueError, match="no extended kernel yet"):
            cls(device="cpu").load(path)


def test_evaluate_and_compare_two_hand_choose_the_class(host, tmp_path, monkeypatch, capsys):
    import evaluation.evaluate as EV
    from agents.greedy import TwoHandPlanAgent, TwoHandShapeAgent, two_hand_agent_class
    from evaluation.tune import compare_two_hand

    evaluate_agent = EV.evaluate_agent  # the real one, before main()'s is stubbed
    assert two_hand_agent_class(None) is TwoHandPlanAgent and two_hand_agent_class({"lines": 5}) is TwoHandPlanAgent
    assert two_hand_agent_class({"lines": 5, **ZEROS}) is TwoHandPlanAgent
    assert two_hand_agent_class({"room5": -1}) is TwoHandShapeAgent
    shaped, plain = str(tmp_path / "s.json"), str(tmp_path / "p.json")
    json.dump({"agent": "plan", "depth": 3, "weights": SHAPED}, open(shaped, "w"))
    json.dump({"agent": "plan", "depth": 3, "weights": X.SETS["zero4"]}, open(plain, "w"))
    built = []
    monkeypatch.setattr(EV, "evaluate_agent", lambda agent, **kw: built.append(agent) or {})
    monkeypatch.setattr(EV, "print_results", lambda res: None)
    for argv in (["--weights", shaped], ["--weights", plain], []):
        monkeypatch.setattr("sys.argv", ["evaluate.py", "--agent", "plan2", "--device", "cpu", "--depth", "2",
                                         "--candidates", "3", "--deals", "2", *argv])
        EV.main()
    assert [type(a) for a in built] == [TwoHandShapeAgent, TwoHandPlanAgent, TwoHandPlanAgent]
    assert built[0].weights["perimeter"] == -3 and (built[0].depth, built[0].candidates, built[0].deals) == (2, 3, 2)
    # tune.py --compare ... --agent plan2: per weight set, and the records are the per-agent evaluations
    recs = compare_two_hand([X.SETS["zero4"], SHAPED], 2, 10, 5, depth=2, candidates=2, deals=2, device="cpu")
    for w, rec in zip((X.SETS["zero4"], SHAPED), recs):
        agent = two_hand_agent_class(w)(w, depth=2, candidates=2, deals=2, seed=5, device="cpu")
        one = evaluate_agent(agent, num_episodes=2, seeds=[5, 6], max_moves=10)
        assert rec["mean_score"] == pytest.approx(float(np.mean(one["scores"])))


class _Positions:
    """What ``PPOAgent.distill`` reads of a buffer: minibatches of stored positions (the network input is not used
    by the stubbed step below)."""

    def __init__(self, board, hand, combo, bs):
        self.cols, self.bs = (board, hand, combo), bs

    def get_position_minibatches(self, batch_size):
        board, hand, combo = self.cols
        for lo in range(0, board.numel(), self.bs):
            s = slice(lo, lo + self.bs)
            yield None, None, board[s].contiguous(), hand[s].contiguous(), combo[s].contiguous()


def test_distill_labels_with_plan_values_ext_on_the_cpu(host, monkeypatch):
    """``PPOAgent.distill`` on device "cpu" over a 64-position buffer: the labelling runs on the host backend; the
    optimizer step is stubbed (it is the fused loss kernel's on the GPU), so what is checked is the q every minibatch
    is labelled with, and the call that made it."""
    from agents.ppo import PPOAgent
    from runtime import kernels as K

    ref = R.reference()
    board, hand, combo = (t[:64].contiguous() for t in R.tensors(ref, torch.device("cpu"))[:3])
    agent = PPOAgent(device=torch.device("cpu"))
    got = []
    monkeypatch.setattr(agent, "distill_minibatch", lambda x, mb, q, tau: got.append(q.clone()) or torch.zeros(6))
    monkeypatch.setattr(agent, "check_optimizer_guard", lambda: None)
    seen = _calls(monkeypatch)
    buf = _Positions(board, hand, combo, 32)
    weights = {**R.DEFAULT_WEIGHTS, **SHAPED}
    agent.distill(buf, weights, depth=2, tau=500.0, epochs=1, batch_size=32)
    want = K.plan_values_ext(board, hand, K.eval_rows(weights), 2, combo=combo, want=("q",))["q"]
    assert len(got) == 2 and torch.equal(torch.cat(got), want)
    assert set(seen[:2]) == {"kernels.plan_values_ext"}
    # the shape weights at 0, or not named: the call made before, under the eight
    for w in ({**R.DEFAULT_WEIGHTS, **ZEROS}, dict(R.DEFAULT_WEIGHTS)):
        del got[:], seen[:]
        agent.distill(buf, w, depth=2, tau=50.0, epochs=1, batch_size=32)
        base = K.plan_values(board, hand, R.DEFAULT_WEIGHTS, 2, combo=combo, want=("q",))["q"]
        assert torch.equal(torch.cat(got), base) and set(seen[:2]) == {"kernels.plan_values"}
    assert not torch.equal(want, base)
    with pytest.raises(ValueError, match="unknown evaluation weights"):
        PPOAgent.search_labeller({"room4": 1, "fits": 2}, 2)
