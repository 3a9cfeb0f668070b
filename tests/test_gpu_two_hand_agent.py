"""``TwoHandPlanAgent`` on the MI355X: 8 envs x 12 moves with three candidates and two deals choose, move for move,
the actions the host backend's agent chooses on the same seeds (tests/test_two_hand_agent_host.py holds that agent to
a plain-Python restatement), and ``evaluate_agent`` plays it.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _play(device, moves=12):
    from agents.greedy import TwoHandPlanAgent
    from runtime.device_env import DeviceEnvBatch

    agent = TwoHandPlanAgent(candidates=3, deals=2, seed=5, device=device)
    env = DeviceEnvBatch(8, [2, 3, 5, 7, 11, 13, 17, 19], autoreset=False, device=device)
    env.reset()
    act = torch.zeros(8, dtype=torch.int32, device=agent.device)
    plain = torch.zeros_like(act)
    log, differs = [], 0
    for _ in range(moves):
        env.plan_actions(plain, agent.weights, agent.depth)
        agent.act_env(env, act)
        differs += int((plain != act).sum())
        log.append(act.cpu().tolist())
        env.step(act)
    score = env.state()["score"].tolist()
    env.close()
    return log, score, differs


def test_actions_equal_the_host_backends(cuda):
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    want, want_score, _ = _play("cpu")
    got, got_score, differs = _play(cuda)
    assert got == want and got_score == want_score
    assert len({tuple(m) for m in got}) > 6 and differs >= 1  # the games move, and the look past the refill matters


def test_evaluate_agent_plays_it(cuda):
    from agents.greedy import HandPlanAgent, TwoHandPlanAgent
    from evaluation.evaluate import evaluate_agent

    one = evaluate_agent(TwoHandPlanAgent(candidates=1, deals=2, device=cuda), num_episodes=4, seed=9, max_moves=18)
    plan = evaluate_agent(HandPlanAgent(device=cuda), num_episodes=4, seed=9, max_moves=18)
    assert one["scores"] == plan["scores"] and one["lengths"] == plan["lengths"]
