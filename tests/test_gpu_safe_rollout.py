"""Training under the hand-safe mask on the MI355X: ``DeviceRollout(..., safe_mask=True)`` and
``training.safe_mask``.

* 64 envs x 48 steps, untrained eval-mode agent: every stored action's bit is set in the stored mask row, every
  stored mask row is the mode-1 reference of the stored board and hand, the mid-hand rule holds; the control without
  the flag ends games in the middle of a hand and fills its buffers bit for bit like a DeviceRollout built without
  the keyword.  (The PPO agent samples through HIP kernels only, so this cannot run on the host backend.)
* 512 envs x 16 steps, eval and train mode (dropout 0): ``collect(graph=True)`` with the flag fills every buffer
  field exactly like the eager loop, over four collects.
* 1,024 envs x 48 steps replayed through the C oracle: board, hand, reward bits, dones and final scores are equal,
  the stored mask rows are the mode-1 reference built from the oracle's legal words and the host backend's safe
  words on the oracle's boards, the mid-hand rule holds and one update on that buffer is finite with entropy > 0;
  the control without the flag has the oracle's mask rows and ends games in the middle of a hand.
* ``train()`` with ``training.safe_mask: true`` logs reward_per_step and mid_hand_losses; without the key it logs
  the key set it always did.

The mid-hand rule: a game that ends on a move that was not its hand's third had, earlier in the same hand, a step
whose stored mask was the fallback (legal moves, none of them safe).
"""
import json

import numpy as np
import pytest
import torch

import _safe_positions as S
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

FIELDS = ("board", "hand", "mask_bits", "actions", "log_probs", "values", "rewards", "dones")


@pytest.fixture(autouse=True)
def repeatable_convolutions():
    """At batches of 64 and 512 MIOpen's forward convolutions are not repeatable run to run in their last bits
    (log-probabilities and values of two identical plain rollouts differ by ~1e-6; at 2,048, the size of
    tests/test_gpu_graph_rollout.py, they are) unless cudnn.deterministic is set, which is what
    ``training.deterministic`` does.  The bit-for-bit comparisons below need it."""
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


def _stored(roll):
    torch.cuda.synchronize()
    buf = roll.buffer
    return {"board": buf.board.cpu().numpy().view(np.uint64), "hand": buf.hand.cpu().numpy().view(np.uint32),
            "mask": buf.mask_bits.cpu().numpy().view(np.uint64), "actions": buf.actions.cpu().numpy().astype(np.int64),
            "dones": buf.dones.cpu().numpy()}


def _action_bits(mask, acts):
    T, n = acts.shape
    return (mask[np.arange(T)[:, None], np.arange(n)[None, :], acts >> 6] >> (acts & 63).astype(np.uint64)) & np.uint64(1)


def _safe_legal(board, hand):
    T, n = board.shape
    safe, legal = S.host_safe_legal(board.reshape(-1), hand.reshape(-1))
    return safe.reshape(T, n, 3), legal.reshape(T, n, 3)


def _mid_hand_terminations(st):
    used = (st["hand"].astype(np.int64) >> 18) & 7
    return int(((st["dones"] > 0) & ~np.isin(used, (3, 5, 6))).sum())


def test_small_rollout_samples_under_the_stored_sampling_mask(cuda):
    from training.trainer import DeviceRollout

    n, T = 64, 48
    rolls = {"safe": DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True),
             "legal": DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=False),
             "plain": DeviceRollout(n, 0, n, 42, {}, T, cuda)}
    for name, r in rolls.items():
        r.reset()
        r.collect(_agent(cuda))
    st = _stored(rolls["safe"])
    assert _action_bits(st["mask"], st["actions"]).all(), "an action outside the stored mask was sampled"
    safe, legal = _safe_legal(st["board"], st["hand"])
    want = S.sampling(safe.reshape(-1, 3), legal.reshape(-1, 3)).reshape(T, n, 3)
    assert np.array_equal(st["mask"], want), "stored mask rows are not the mode-1 words of the stored positions"
    mid = S.mid_hand_rule(st["hand"], st["dones"], st["mask"], (safe, legal))
    print(f"safe rollout {n} x {T}: {int((st['dones'] > 0).sum())} episodes ended, {mid} in the middle of a hand")
    assert mid == 0  # none is expected at this size
    ctl = _stored(rolls["legal"])
    assert _mid_hand_terminations(ctl) > 0, "the control never lost in the middle of a hand: the test shows nothing"
    for f in FIELDS:
        assert torch.equal(getattr(rolls["legal"].buffer, f), getattr(rolls["plain"].buffer, f)), f
    for r in rolls.values():
        r.close()


@pytest.mark.parametrize("train_mode", [False, True])
def test_graph_rollout_with_the_flag_equals_eager(cuda, train_mode):
    from training.trainer import DeviceRollout

    n, T = 512, 16
    a_eager, a_graph = _agent(cuda, train_mode), _agent(cuda, train_mode)
    a_graph.network.load_state_dict(a_eager.network.state_dict())
    r_eager, r_graph = (DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=True) for _ in range(2))
    for r in (r_eager, r_graph):
        r.reset()
    for it in range(4):  # warm-up (eager), capture + replay, replay, replay
        r_eager.collect(a_eager)
        r_graph.collect(a_graph, graph=True)
        torch.cuda.synchronize(cuda)
        for f in FIELDS:
            assert torch.equal(getattr(r_eager.buffer, f), getattr(r_graph.buffer, f)), f"rollout {it}: {f} differs"
        assert a_eager.sample_step == a_graph.sample_step == (it + 1) * T
        assert (r_graph._graph is not None) == (it >= 1)
    assert r_graph._graph_key[-1] is True
    legal = torch.zeros((n, 3), dtype=torch.int64, device=cuda)
    assert any(not torch.equal(r_graph.buffer.mask_bits[t], legal) for t in range(T))
    se, sg = r_eager.env.state(), r_graph.env.state()
    for k in se:
        assert (se[k] == sg[k]).all(), k
    for r in (r_eager, r_graph):
        r.close()


def _oracle_replay(roll, n, label, safe_mask):
    cpu = CO.CVecEnv(np.arange(42, 42 + n, dtype=np.uint64))
    cpu.reset()
    st = _stored(roll)
    ref = cpu.replay(st["actions"].astype(np.int32))
    buf = roll.buffer
    assert np.array_equal(st["board"], ref["board"]), f"{label}: board snapshots"
    assert np.array_equal(st["hand"], ref["hand"]), f"{label}: hand snapshots"
    assert np.array_equal(buf.rewards.cpu().numpy().view(np.uint32), ref["reward"].view(np.uint32)), f"{label}: rewards"
    assert np.array_equal(st["dones"], ref["terminated"].astype(np.float32)), f"{label}: dones"
    d = st["dones"] > 0
    assert np.array_equal(roll.ep_score.cpu().numpy()[d], ref["ep_score"][d]), f"{label}: final scores"
    T = st["actions"].shape[0]
    if safe_mask:
        safe, _ = _safe_legal(ref["board"], ref["hand"])  # the host backend's safe words on the oracle's boards
        legal = ref["mask"].reshape(T, n, 3)                # the oracle's legal words
        want = S.sampling(safe.reshape(-1, 3), legal.reshape(-1, 3)).reshape(T, n, 3)
        assert np.array_equal(st["mask"], want), f"{label}: stored mask rows against the mode-1 reference"
        mid = S.mid_hand_rule(st["hand"], st["dones"], st["mask"], (safe, legal))
    else:
        assert np.array_equal(st["mask"], ref["mask"].reshape(T, n, 3)), f"{label}: mask snapshots"
        mid = _mid_hand_terminations(st)
    assert _action_bits(st["mask"], st["actions"]).all(), f"{label}: an action outside the stored mask"
    cpu.close()
    return int(d.sum()), mid


def test_safe_rollout_replays_through_the_c_oracle(cuda):
    from training.trainer import DeviceRollout

    n, T = 1024, 48
    for flag in (True, False):
        torch.manual_seed(42)
        agent = _agent(cuda, train_mode=True, seed=42, sample_seed=7)
        roll = DeviceRollout(n, 0, n, 42, {}, T, cuda, safe_mask=flag)
        roll.reset()
        roll.collect(agent)
        ended, mid = _oracle_replay(roll, n, f"safe_mask={flag}", flag)
        print(f"safe_mask={flag}: {n} envs x {T} steps bit-exact against the oracle, {ended} episodes ended, "
              f"{mid} in the middle of a hand")
        if flag:
            agent.config.num_epochs = 1
            m = agent.update(roll.buffer, agent.values_device(roll.x))
            assert all(np.isfinite(v) for v in m.values()), m
            assert m["entropy"] > 0
        else:
            assert mid > 0, "the control never lost in the middle of a hand"
        roll.close()


def test_train_logs_the_two_keys_only_under_the_flag(cuda, tmp_path, capsys):
    from training import train

    recs = {}
    for flag in (True, False):
        tmp = tmp_path / str(flag)
        cfg = {"ppo": {"num_epochs": 1},
               "training": {"num_envs": 256, "batch_size": 1024, "rollout_steps": 16, "total_timesteps": 10 ** 9},
               "rewards": {}, "logging": {"log_interval": 1, "save_interval": 1000},
               "paths": {"checkpoint_dir": str(tmp / "ck"), "log_dir": str(tmp / "logs"),
                         "results_dir": str(tmp / "res")}}
        if flag:
            cfg["training"]["safe_mask"] = True
        s = train(cfg, seed=42, max_updates=2)
        assert s["updates"] == 2
        said = "hand-safe mask" in capsys.readouterr().out
        assert said == flag
        logs = list((tmp / "logs").glob("ppo_*.jsonl"))
        assert len(logs) == 1
        recs[flag] = [json.loads(x) for x in logs[0].read_text().splitlines()]
        assert len(recs[flag]) == 2
    new = {"reward_per_step", "mid_hand_losses"}
    for r in recs[True]:
        assert new <= set(r) and np.isfinite(r["reward_per_step"]) and r["mid_hand_losses"] >= 0
        assert float(r["mid_hand_losses"]) == int(r["mid_hand_losses"])
    today = {"step", "fps", "avg_score", "max_score", "best_score", "avg_length", "policy_loss", "value_loss", "entropy",
             "total_loss", "approx_kl", "clip_fraction"}
    for r in recs[False]:
        assert not (new & set(r)) and today <= set(r)
        assert set(r) == set(recs[True][0]) - new
