"""Distillation training on the MI355X: ``DeviceRollout(..., positions=True)``, ``PPOAgent.distill_minibatch`` /
``distill`` and ``training.distill``.

* 256 envs x 8 steps under the hand-safe mask with ``positions=True``: the stored combo rows are the combos of the
  same games replayed through the host backend (boards and hands too, so the replay is the same game), and
  ``collect(graph=True)`` fills every field, combo included, like the eager loop over four collects.
* Overfit: 40 ``distill_minibatch`` steps on one fixed minibatch of 512 stored positions (q from
  bb_plan_values_pos at depth 2) lower the eval-mode cross-entropy on that minibatch and do not lower the
  agreement -- a condition on a repeated batch, not a measured threshold.
* A distill step leaves every value-head parameter bit-unchanged.
* ``train()`` with ``distill.updates: 1`` for two iterations: the first log record carries the five distill keys,
  the second PPO's, and the checkpoint loads.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ("board", "hand", "mask_bits", "combo", "actions", "log_probs", "values", "rewards", "dones")


@pytest.fixture(autouse=True)
def repeatable_convolutions():
    """As tests/test_gpu_safe_rollout.py: at these batch sizes MIOpen's forward convolutions repeat bit for bit only
    under cudnn.deterministic, which the eager / captured comparison needs."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _agent(cuda, train_mode=False, seed=3, sample_seed=77):
    from agents import PPOAgent, PPOConfig

    torch.manual_seed(seed)
    a = PPOAgent(PPOConfig(), cuda, sample_seed=sample_seed)
    if train_mode:
        a.train()
        for m in a.network.modules():  # dropout off: its torch RNG stream differs under capture
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    else:
        a.eval()
    return a


def test_stored_combo_is_the_host_replay(cuda):
    from runtime.device_env import DeviceEnvBatch
    from training.trainer import DeviceRollout

    n, T = 256, 8
    roll = DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True, positions=True)
    roll.reset()
    agent = _agent(cuda)
    seen = set()
    host = DeviceEnvBatch(n, [42 + i for i in range(n)], {}, autoreset=True, device="cpu")
    host.reset()
    for it in range(3):  # combos build up over the later rollouts
        roll.collect(agent)
        torch.cuda.synchronize(cuda)
        buf = roll.buffer
        combo, board = buf.combo.cpu().numpy(), buf.board.cpu().numpy().view(np.uint64)
        acts = buf.actions.cpu().to(torch.int32)
        for t in range(T):
            st = host.state()
            assert np.array_equal(board[t], st["board"]), (it, t)
            assert np.array_equal(combo[t], st["combo"]), (it, t)
            seen |= set(st["combo"].tolist())
            host.step(acts[t].contiguous())
    assert len(seen) > 1, "combo never moved: the test shows nothing"
    host.close()
    roll.close()


def test_graph_rollout_with_positions_equals_eager(cuda):
    from training.trainer import DeviceRollout

    n, T = 256, 8
    a_eager, a_graph = _agent(cuda), _agent(cuda)
    a_graph.network.load_state_dict(a_eager.network.state_dict())
    r_eager, r_graph = (DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True, positions=True) for _ in range(2))
    for r in (r_eager, r_graph):
        r.reset()
    moved = False
    for it in range(4):  # warm-up (eager), capture + replay, replay, replay
        r_eager.collect(a_eager)
        r_graph.collect(a_graph, graph=True)
        torch.cuda.synchronize(cuda)
        for f in FIELDS:
            assert torch.equal(getattr(r_eager.buffer, f), getattr(r_graph.buffer, f)), f"rollout {it}: {f} differs"
        assert (r_graph._graph is not None) == (it >= 1)
        moved = moved or bool(r_graph.buffer.combo.any())
    assert moved, "combo never moved: the test shows nothing"
    assert r_graph._graph_key[-2:] == (True, True)  # (positions, safe_mask)
    plain = DeviceRollout(n, 0, n, 42, {}, T, cuda)
    assert not hasattr(plain.buffer, "combo") and plain.positions is False
    for r in (r_eager, r_graph, plain):
        r.close()


@pytest.fixture(scope="module")
def stored_minibatch(cuda):
    """One minibatch of 512 stored positions of a 256 x 8 safe rollout with its depth-2 search values."""
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K
    from training.trainer import DeviceRollout

    n, T = 256, 8
    roll = DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True, positions=True)
    roll.reset()
    agent = _agent(cuda)
    for _ in range(2):
        roll.collect(agent)
    gen = torch.Generator(device=cuda)
    gen.manual_seed(5)
    x, mb, board, hand, combo = next(roll.buffer.get_position_minibatches(512, gen))
    q = K.plan_values(board, hand, DEFAULT_WEIGHTS, 2, combo=combo, want=("q",))["q"]
    torch.cuda.synchronize(cuda)
    legal = q != torch.iinfo(torch.int64).min
    assert bool((K.mask_bits_to_bool(mb) & ~legal).sum() == 0)  # the stored mask is within the search's legal set
    out = tuple(t.clone() for t in (x, mb, q))
    roll.close()
    return out


def _eval_stats(agent, x, mb, q, tau):
    from runtime import kernels as K

    agent.eval()
    with torch.no_grad():
        _, stats = K.distill_loss(agent._raw(x)[0], mb, q, tau)
    agent.train()
    return stats.cpu().numpy()


def test_forty_steps_overfit_one_minibatch(cuda, stored_minibatch):
    x, mb, q = stored_minibatch
    agent = _agent(cuda, train_mode=True, seed=9)
    tau = 50.0
    before = _eval_stats(agent, x, mb, q, tau)
    for _ in range(40):
        st = agent.distill_minibatch(x, mb, q, tau)
    torch.cuda.synchronize(cuda)
    assert st.shape == (6,) and bool(torch.isfinite(st).all())
    after = _eval_stats(agent, x, mb, q, tau)
    print(f"overfit 512 positions, 40 steps: ce {before[0]:.4f} -> {after[0]:.4f}, kl {before[1]:.4f} -> "
          f"{after[1]:.4f}, agreement {before[4]:.4f} -> {after[4]:.4f}, rows {int(after[5])}")
    assert before[5] == after[5] > 0
    assert after[0] < before[0]
    assert after[4] >= before[4]
    agent.check_optimizer_guard()


@pytest.mark.parametrize("bf16", [False, True])
def test_value_head_is_untouched_by_a_distill_step(cuda, stored_minibatch, bf16):
    x, mb, q = stored_minibatch
    agent = _agent(cuda, train_mode=True, seed=9)
    if bf16:
        agent.autocast_dtype = torch.bfloat16
    net = agent.network
    value = {k: v.detach().clone() for k, v in net.value_head.state_dict().items()}
    policy = {k: v.detach().clone() for k, v in net.policy_head.state_dict().items()}
    agent.distill_minibatch(x, mb, q, 50.0)
    torch.cuda.synchronize(cuda)
    for k, v in net.value_head.state_dict().items():
        assert torch.equal(v, value[k]), k
    assert any(not torch.equal(v, policy[k]) for k, v in net.policy_head.state_dict().items())


def test_train_distills_first_then_ppo(cuda, tmp_path, capsys):
    from agents import PPOAgent, PPOConfig
    from agents.ppo import DISTILL_KEYS
    from training import train

    cfg = {"ppo": {"num_epochs": 1},
           "training": {"num_envs": 256, "batch_size": 1024, "rollout_steps": 16, "total_timesteps": 2 * 256 * 16,
                        "safe_mask": True, "distill": {"updates": 1, "depth": 2}},
           "rewards": {}, "logging": {"log_interval": 1, "save_interval": 1000},
           "paths": {"checkpoint_dir": str(tmp_path / "ck"), "log_dir": str(tmp_path / "logs"),
                     "results_dir": str(tmp_path / "res")}}
    s = train(cfg, seed=42)
    assert s["updates"] == 2
    assert capsys.readouterr().out.count("training.distill") == 1
    logs = list((tmp_path / "logs").glob("ppo_*.jsonl"))
    assert len(logs) == 1
    recs = [json.loads(x) for x in logs[0].read_text().splitlines()]
    assert len(recs) == 2
    ppo = {"policy_loss", "value_loss", "entropy", "total_loss", "approx_kl", "clip_fraction"}
    assert set(DISTILL_KEYS) <= set(recs[0]) and not (ppo & set(recs[0]))
    assert all(np.isfinite(recs[0][k]) for k in DISTILL_KEYS)
    assert recs[0]["distill_ce"] > 0 and 0 <= recs[0]["distill_agreement"] <= 1
    assert ppo <= set(recs[1]) and not (set(DISTILL_KEYS) & set(recs[1]))
    agent = PPOAgent(PPOConfig(), cuda)
    agent.load(str(tmp_path / "ck" / "final.pt"))
