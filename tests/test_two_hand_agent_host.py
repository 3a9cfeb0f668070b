"""``TwoHandPlanAgent`` on the host backend (CPU): with one candidate it plays ``HandPlanAgent``'s games move for move,
and with three candidates and two deals every action equals a restatement of the agent's six steps in plain Python on
the references (tests/_plan_values_ref.py for q and rest, the oracle env for the leaf, tests/_refill_values_ref.py for
the dealt values), which calls none of bb_plan_values, bb_play_plan_pos or bb_refill_values.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _plan_values_ref as PV
import _play_plan_ref as PP
import _refill_values_ref as RV

INT64_MIN = R.INT64_MIN


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


def _games(n, seeds):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(n, list(seeds), autoreset=False, device="cpu")
    env.reset()
    return env


def test_one_candidate_plays_the_hand_plan_agent(host):
    from agents.greedy import HandPlanAgent, TwoHandPlanAgent

    seeds = [3, 5, 8, 13]
    logs = []
    for agent in (HandPlanAgent(device="cpu"), TwoHandPlanAgent(candidates=1, deals=3, seed=9, device="cpu")):
        env = _games(4, seeds)
        act = torch.zeros(4, dtype=torch.int32)
        log = []
        for _ in range(30):
            agent.act_env(env, act)
            log.append(act.tolist())
            env.step(act)
        logs.append(log)
        env.close()
    assert logs[0] == logs[1]
    assert len({tuple(m) for m in logs[0]}) > 10  # the games move


def restated_actions(state, weights, depth, candidates, deals, seed, move):
    """Steps 1-6 of ``TwoHandPlanAgent`` for the envs of ``state`` (DeviceEnvBatch.state()), in plain Python."""
    board, hand, combo = state["board"], state["hand"], state["combo"]
    n = len(board)
    per = PV.per_action(board, hand, combo, depth)                       # step 1
    q, rest = per["q"]["default"], per["rest"]["default"]
    key = (int(seed) + (move + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
    rows = []  # (env, action, leaf) of every candidate
    for i in range(n):
        legal = [a for a in range(192) if q[i, a] != INT64_MIN]
        for a in sorted(legal, key=lambda a: (-int(q[i, a]), a))[:candidates]:  # step 2
            a2, a3 = int(rest[i, a]) & 0xFF, (int(rest[i, a]) >> 8) & 0xFF
            env = R.make_env(int(board[i]), [(int(hand[i]) >> (6 * s)) & 63 for s in range(3)],
                             used=[bool((int(hand[i]) >> (18 + s)) & 1) for s in range(3)], combo=int(combo[i]))
            rows.append((i, a, PP.oracle_play(env, [a, -1 if a2 == 0xFF else a2, -1 if a3 == 0xFF else a3])))  # step 3
    q2 = {}
    refills = [(i, a, leaf) for i, a, leaf in rows if leaf[5] & PP.REFILL]
    if refills:                                                         # step 4
        ref = RV.refill_values(np.array([leaf[0] for _, _, leaf in refills], np.uint64), deals, key, depth, weights,
                               combo=[leaf[2] for _, _, leaf in refills], stream=[i for i, _, _ in refills])
        for (i, a, leaf), values in zip(refills, ref["value"]):
            moved = weights["lines"] * leaf[3] + weights["score"] * leaf[4]
            q2[i, a] = deals * moved + int(values.sum())
    for i, a, leaf in rows:                                             # step 5
        q2.setdefault((i, a), deals * int(q[i, a]))
    actions = []
    for i in range(n):                                                  # step 6
        mine = [(v, -a) for (e, a), v in q2.items() if e == i]
        actions.append(-max(mine)[1] if mine else 0)
    return actions, len(refills), len(rows) - len(refills)


@pytest.mark.parametrize("depth,games,moves", [(2, 3, 12), (3, 2, 3)])
def test_three_candidates_two_deals_against_the_restatement(host, depth, games, moves):
    from agents.greedy import DEFAULT_WEIGHTS, TwoHandPlanAgent

    assert DEFAULT_WEIGHTS == R.DEFAULT_WEIGHTS  # per_action's "default" set is the agent's
    agent = TwoHandPlanAgent(depth=depth, candidates=3, deals=2, seed=77, device="cpu")
    env = _games(games, [21, 34, 55][:games])
    act = torch.zeros(games, dtype=torch.int32)
    refills = others = differs = 0
    for move in range(moves):
        want, r, o = restated_actions(env.state(), DEFAULT_WEIGHTS, depth, 3, 2, 77, move)
        plain = torch.zeros(games, dtype=torch.int32)
        env.plan_actions(plain, DEFAULT_WEIGHTS, depth)
        agent.act_env(env, act)
        assert act.tolist() == want, move
        refills, others, differs = refills + r, others + o, differs + int((plain != act).sum())
        env.step(act)
    env.close()
    assert agent.moves == moves and refills >= 6
    if depth == 2:
        assert others >= 6 and differs >= 1  # leaves cut by the depth keep q; the look past the refill changes a move


def test_the_agent_refuses_bad_settings(host):
    from agents.greedy import TwoHandPlanAgent

    for kw in (dict(candidates=0), dict(candidates=193), dict(deals=0), dict(deals=1025), dict(depth=4)):
        with pytest.raises(ValueError):
            TwoHandPlanAgent(device="cpu", **kw)
    assert TwoHandPlanAgent.deal_seed(2 ** 64 - 1, 0) == (2 ** 64 - 1 + 0x9E3779B97F4A7C15) % 2 ** 64


def test_save_and_load_keep_the_settings(host, tmp_path):
    from agents.greedy import TwoHandPlanAgent

    a = TwoHandPlanAgent({"holes": -7}, depth=2, candidates=5, deals=9, seed=4, device="cpu")
    a.save(str(tmp_path / "a.json"))
    b = TwoHandPlanAgent(device="cpu")
    b.load(str(tmp_path / "a.json"))
    assert (b.depth, b.candidates, b.deals, b.seed, b.weights) == (2, 5, 9, 4, a.weights)
