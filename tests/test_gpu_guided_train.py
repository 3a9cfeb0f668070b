"""Search-guided PPO training on the MI355X: ``PackedRolloutBuffer.get_guided_minibatches``,
``PPOAgent.guided_minibatch`` / ``update_guided`` and ``training.distill.value_coef`` / ``training.guide``.

All on a 256 envs x 8 steps rollout under the hand-safe mask with ``positions=True`` (2,048 stored positions, four
minibatches of 512), q from bb_plan_values_pos at depth 2, under cudnn.deterministic as tests/test_gpu_distill_train.py.

* The guided minibatches are the rows of ``get_minibatches`` and ``get_position_minibatches`` under the same generator.
* The captured ``guided_minibatch`` equals the eager one over four steps, and with distill_coef = 0 and PPOConfig's
  coefficients it leaves the weights ``train_minibatch`` leaves: both at the tolerance of
  test_graphed_minibatch_step_matches_eager in tests/test_gpu_ppo_agent.py (statistics 1e-4 on the first step, 2e-3
  later; weights 4 lr; buffers 1e-3).
* 40 steps on one fixed minibatch with coefficients (policy 0, value 0.5, entropy 0, distill 1): the eval-mode
  cross-entropy and value loss both end strictly lower than they began, and the value head's parameters change -- a
  condition on a repeated batch, not a measured threshold.
* Changing the coefficients between two replays does not re-capture.
* ``train()`` with ``distill.updates: 1``, ``value_coef`` and a ``guide`` block: the log carries the distillation
  iteration's keys first, then the PPO keys plus DISTILL_KEYS and guide_beta, and the checkpoint loads.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PPO_KEYS = ("policy_loss", "value_loss", "entropy", "total_loss", "approx_kl", "clip_fraction")


@pytest.fixture(autouse=True)
def repeatable_convolutions():
    """As tests/test_gpu_distill_train.py: at these batch sizes MIOpen's forward convolutions repeat bit for bit only
    under cudnn.deterministic, which the eager / captured comparison needs."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _agent(cuda, seed=3, graphs=True):
    from agents import PPOAgent, PPOConfig

    torch.manual_seed(seed)
    a = PPOAgent(PPOConfig(batch_size=512), cuda, sample_seed=77)
    a.train()
    for m in a.network.modules():  # dropout off: its torch RNG stream differs under capture
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    a.use_graphs = graphs
    return a


@pytest.fixture(scope="module")
def stored(cuda):
    """The four guided minibatches of 512 stored positions of a 256 x 8 safe rollout, each with its depth-2 search
    values appended: (x, mask_bits, actions, old_logp, adv, ret, q)."""
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K
    from training.trainer import DeviceRollout

    n, T = 256, 8
    roll = DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True, positions=True)
    roll.reset()
    agent = _agent(cuda)
    agent.eval()
    for _ in range(2):
        roll.collect(agent)
    buf = roll.buffer
    buf.compute_returns_and_advantages(agent.values_device(roll.x), 0.99, 0.95)

    def gen():
        g = torch.Generator(device=cuda)
        g.manual_seed(5)
        return g

    guided = [tuple(t.clone() for t in b) for b in buf.get_guided_minibatches(512, gen())]
    ppo = [tuple(t.clone() for t in b) for b in buf.get_minibatches(512, gen())]
    pos = [tuple(t.clone() for t in b) for b in buf.get_position_minibatches(512, gen())]
    assert len(guided) == len(ppo) == len(pos) == 4
    for gb, pb, qb in zip(guided, ppo, pos):  # the rows of both existing iterators
        assert torch.equal(gb[0], pb[0]) and torch.equal(gb[0], qb[0])
        assert torch.equal(K.mask_bits_to_bool(gb[1]).float(), pb[1]) and torch.equal(gb[1], qb[1])
        assert all(torch.equal(a, b) for a, b in zip(gb[2:6], pb[2:6]))
        assert all(torch.equal(a, b) for a, b in zip(gb[6:9], qb[2:5]))
    out = []
    for x, mb, a, lp, adv, ret, board, hand, combo in guided:
        q = K.plan_values(board, hand, DEFAULT_WEIGHTS, 2, combo=combo, want=("q",))["q"]
        legal = q != torch.iinfo(torch.int64).min
        assert bool((K.mask_bits_to_bool(mb) & ~legal).sum() == 0)  # the stored mask is within the search's legal set
        out.append((x, mb, a, lp, adv, ret, q.clone()))
    torch.cuda.synchronize(cuda)
    roll.close()
    return out


def _close(eager, other, lr):
    for (n1, p1), p2 in zip(eager.network.named_parameters(), other.network.parameters()):
        assert torch.allclose(p1, p2, rtol=0, atol=4 * lr), n1
    for b1, b2 in zip(eager.network.buffers(), other.network.buffers()):
        assert torch.allclose(b1.float(), b2.float(), rtol=1e-3, atol=1e-3)


def test_captured_guided_step_matches_eager(cuda, stored):
    eager, graphed = _agent(cuda, graphs=False), _agent(cuda)
    coefs = (1.0, 0.5, 0.01, 0.3, 50.0)
    for k, b in enumerate(stored):
        s_e = eager.guided_minibatch(*b, coefs).clone()
        s_g = graphed.guided_minibatch(*b, coefs).clone()
        tol = 1e-4 if k == 0 else 2e-3
        assert s_e.shape == (12,) and torch.allclose(s_e, s_g, rtol=tol, atol=tol), (k, s_e, s_g)
    assert len(graphed._graphs) == 1 and len(eager._graphs) == 0
    _close(eager, graphed, eager.config.learning_rate)
    assert int(graphed.optimizer.state[next(graphed.network.parameters())]["step"]) == len(stored)
    graphed.check_optimizer_guard()


def test_guided_step_without_distillation_is_the_ppo_step(cuda, stored):
    from runtime import kernels as K

    ppo, guided = _agent(cuda), _agent(cuda)
    cfg = ppo.config
    coefs = (1.0, cfg.value_coef, cfg.entropy_coef, 0.0, 50.0)
    for k, (x, mb, a, lp, adv, ret, q) in enumerate(stored):
        s_p = ppo.train_minibatch(x, K.mask_bits_to_bool(mb).float(), a, lp, adv, ret).clone()
        s_g = guided.guided_minibatch(x, mb, a, lp, adv, ret, q, coefs).clone()
        tol = 1e-4 if k == 0 else 2e-3
        assert torch.allclose(s_p, s_g[:6], rtol=tol, atol=tol), (k, s_p, s_g)
    _close(ppo, guided, cfg.learning_rate)


def _eval_stats(agent, batch, coefs):
    from runtime import kernels as K

    x, rest = batch[0], batch[1:]
    agent.eval()
    with torch.no_grad():
        logits, values = agent._raw(x)
        _, stats = K.guided_loss(logits, values, *rest, agent.config.clip_epsilon, coefs)
    agent.train()
    return stats.cpu().numpy()


def test_forty_steps_fit_the_policy_and_the_critic(cuda, stored):
    agent = _agent(cuda, seed=9)
    coefs = (0.0, 0.5, 0.0, 1.0, 50.0)
    batch = stored[0]
    value = {k: v.detach().clone() for k, v in agent.network.value_head.state_dict().items()}
    before = _eval_stats(agent, batch, coefs)
    for _ in range(40):
        st = agent.guided_minibatch(*batch, coefs)
    torch.cuda.synchronize(cuda)
    assert st.shape == (12,) and bool(torch.isfinite(st).all())
    after = _eval_stats(agent, batch, coefs)
    print(f"\n512 positions, 40 steps: ce {before[6]:.4f} -> {after[6]:.4f}, value_loss {before[1]:.4f} -> "
          f"{after[1]:.4f}, agreement {before[10]:.4f} -> {after[10]:.4f}, rows {int(after[11])}")
    assert before[11] == after[11] > 0
    assert after[6] < before[6] and after[1] < before[1]
    assert any(not torch.equal(v, value[k]) for k, v in agent.network.value_head.named_parameters())
    agent.check_optimizer_guard()


def test_a_schedule_does_not_recapture(cuda, stored):
    agent = _agent(cuda)
    batch = stored[0]
    first = agent.guided_minibatch(*batch, (1.0, 0.5, 0.01, 1.0, 50.0)).clone()
    (key, ent), = agent._graphs.items()
    graph, cdev = ent[0][0], ent[3]
    second = agent.guided_minibatch(*batch, (1.0, 0.5, 0.01, 0.25, 20.0)).clone()
    torch.cuda.synchronize(cuda)
    assert list(agent._graphs) == [key] and agent._graphs[key][0][0] is graph and agent._graphs[key][3] is cdev
    assert cdev.tolist() == pytest.approx([1.0, 0.5, 0.01, 0.25, 20.0])
    # the replay read the new coefficients: total = policy + 0.5 value - 0.01 entropy + 0.25 cross-entropy
    for st, beta in ((first, 1.0), (second, 0.25)):
        s = st.double().cpu().numpy()
        assert s[3] == pytest.approx(s[0] + 0.5 * s[1] - 0.01 * s[2] + beta * s[6], rel=1e-5, abs=1e-6)


def test_update_guided_fills_the_captured_steps_buffers(cuda):
    """update_guided over a rollout: once the step is captured the minibatches are gathered straight into its input
    buffers and the search writes into its q buffer; the 11 keys come back finite."""
    from agents.greedy import DEFAULT_WEIGHTS
    from agents.ppo import DISTILL_KEYS
    from training.trainer import DeviceRollout

    n, T = 256, 8
    roll = DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True, positions=True)
    roll.reset()
    agent = _agent(cuda)
    agent.config.num_epochs = 1
    roll.collect(agent)
    assert agent.guided_inputs(512) is None
    m = agent.update_guided(roll.buffer, agent.values_device(roll.x), DEFAULT_WEIGHTS, 2, 50.0,
                            (1.0, 0.5, 0.01, 0.5), batch_size=512)
    assert list(m) == list(PPO_KEYS + DISTILL_KEYS) and all(np.isfinite(v) for v in m.values())
    assert m["distill_ce"] > 0 and 0 <= m["distill_agreement"] <= 1
    dst = agent.guided_inputs(512)
    (ent,) = agent._graphs.values()
    assert len(dst) == 9 and all(a is b for a, b in zip(dst[:6], ent[1][:6]))
    roll.collect(agent)
    m2 = agent.update_guided(roll.buffer, agent.values_device(roll.x), DEFAULT_WEIGHTS, 2, 50.0,
                             (0.0, 0.5, 0.0, 1.0), batch_size=512, epochs=2)
    assert len(agent._graphs) == 1 and all(np.isfinite(v) for v in m2.values())
    roll.close()


def test_train_distills_with_the_critic_then_guides_ppo(cuda, tmp_path, capsys):
    from agents import PPOAgent, PPOConfig
    from agents.ppo import DISTILL_KEYS
    from training import train

    cfg = {"ppo": {"num_epochs": 1},
           "training": {"num_envs": 256, "batch_size": 1024, "rollout_steps": 16, "total_timesteps": 3 * 256 * 16,
                        "safe_mask": True, "distill": {"updates": 1, "depth": 2, "value_coef": 0.5},
                        "guide": {"beta": 1.0, "beta_final": 0.5, "decay_updates": 1}},
           "rewards": {}, "logging": {"log_interval": 1, "save_interval": 1000},
           "paths": {"checkpoint_dir": str(tmp_path / "ck"), "log_dir": str(tmp_path / "logs"),
                     "results_dir": str(tmp_path / "res")}}
    s = train(cfg, seed=42)
    assert s["updates"] == 3
    out = capsys.readouterr().out
    assert out.count("training.distill") == 1 and out.count("training.guide") == 1
    logs = list((tmp_path / "logs").glob("ppo_*.jsonl"))
    assert len(logs) == 1
    recs = [json.loads(x) for x in logs[0].read_text().splitlines()]
    assert len(recs) == 3
    both = set(PPO_KEYS) | set(DISTILL_KEYS)
    assert both <= set(recs[0]) and "guide_beta" not in recs[0]
    assert recs[0]["value_loss"] > 0 and recs[0]["distill_ce"] > 0
    for r, beta in zip(recs[1:], (1.0, 0.5)):
        assert both <= set(r) and r["guide_beta"] == beta
        assert all(np.isfinite(r[k]) for k in both)
        assert r["distill_ce"] > 0 and 0 <= r["distill_agreement"] <= 1
    agent = PPOAgent(PPOConfig(), cuda)
    agent.load(str(tmp_path / "ck" / "final.pt"))
