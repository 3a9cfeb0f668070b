"""Policy distillation off the GPU: ``agents.ppo.distill_loss_torch`` against the fp64 restatement
(tests/_distill_ref.py), the host backend's bb_snapshot_combo, the rollout buffer's ``positions`` switch, the
trainer's ``training.distill`` switch on a stub agent, and the argument rules of the bb_distill_loss entry points
(checked before any HIP call, so they show without a device)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _distill_ref as R

FAKE = 0x10000  # a host integer standing for a device pointer: validation never dereferences it


@pytest.mark.parametrize("tau", [0.0, 1.0, 50.0, 1e4])
@pytest.mark.parametrize("density", ["one", "tenth", "all", "mixed"])
def test_torch_loss_matches_fp64_restatement(tau, density):
    from agents.ppo import distill_loss_torch

    logits, mb, q = R.synthetic(37, seed=11, density=density)
    want = R.reference(logits, mb, q, tau)
    x = torch.from_numpy(logits).requires_grad_(True)
    loss, stats = distill_loss_torch(x, torch.from_numpy(mb), torch.from_numpy(q), tau)
    loss.backward()
    np.testing.assert_allclose(stats.numpy()[:4], want["stats"][:4], rtol=1e-5, atol=1e-6)
    assert stats[4].item() * 37 == pytest.approx(want["stats"][4] * 37, abs=1e-4)  # a count over 37
    assert stats[5].item() == want["stats"][5]
    assert loss.item() == stats[0].item()
    g = x.grad.numpy()
    np.testing.assert_allclose(g, want["dlogits"], rtol=1e-4, atol=1e-5 * np.abs(want["dlogits"]).max())
    M = R.mask_bool(mb)
    assert not g[~M].any() and not g[~want["has"]].any()
    if tau == 0:  # the one negative entry of a row's gradient is its target: the lowest argmax of q
        rows = np.flatnonzero(want["has"] & (M.sum(axis=1) > 1))
        assert np.array_equal(np.argmin(g[rows], axis=1), want["qarg"][rows])


def test_reference_tie_rules():
    """The restatement's own tie rules on a hand-made row: q ties at 7 on actions 3, 64 and 130, the logits tie at
    their maximum on 64 and 130 -> the teacher's action is 3, the student's 64, no agreement; at tau == 0 the target
    is the one-hot of 3."""
    q = np.full((1, 192), -5, np.int64)
    q[0, [3, 64, 130]] = 7
    logits = np.zeros((1, 192), np.float32)
    logits[0, [64, 130]] = 2.0
    mb = R.mask_words(np.ones((1, 192), bool))
    r = R.reference(logits, mb, q, 0.0)
    assert r["qarg"][0] == 3 and r["parg"][0] == 64 and r["stats"][4] == 0.0
    assert r["t"][0, 3] == 1.0 and r["t"].sum() == 1.0
    r = R.reference(logits, mb, q, 1.0)
    assert r["t"][0, 3] == r["t"][0, 64] == r["t"][0, 130] and abs(r["t"].sum() - 1.0) < 1e-12
    mb = R.mask_words(np.arange(192)[None, :] != 3)  # mask the lowest tied action out: the next one takes over
    assert R.reference(logits, mb, q, 0.0)["qarg"][0] == 64


def test_host_snapshot_combo_equals_state():
    from runtime.device_env import DeviceEnvBatch

    n = 64
    env = DeviceEnvBatch(n, list(range(900, 900 + n)), autoreset=True, device="cpu")
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64)
    act = torch.zeros(n, dtype=torch.int32)
    out = torch.full((n,), -7, dtype=torch.int32)
    seen = set()
    for t in range(60):
        env.obs(mask_bits=mb)
        env.random_actions(mb, act, step=t)
        env.step(act)
        env.snapshot_combo(out)
        want = env.state()["combo"]
        assert np.array_equal(out.numpy(), want), t
        seen |= set(want.tolist())
    assert len(seen) > 1, "combo never moved: the test shows nothing"
    assert env.lib.bb_snapshot_combo(None, out.data_ptr(), None) == -1  # NULL handle: BB_ERR_ARG, as bb_snapshot
    env.close()


def test_buffer_without_positions_is_todays():
    from agents.ppo import PackedRolloutBuffer

    plain = PackedRolloutBuffer(4, 8, torch.device("cpu"))
    off = PackedRolloutBuffer(4, 8, torch.device("cpu"), positions=False)
    on = PackedRolloutBuffer(4, 8, torch.device("cpu"), positions=True)
    assert not hasattr(plain, "combo") and not hasattr(off, "combo")
    assert set(vars(off)) == set(vars(plain))
    assert set(vars(on)) == set(vars(plain)) | {"combo"}
    assert on.combo.dtype == torch.int32 and tuple(on.combo.shape) == (4, 8)
    with pytest.raises(RuntimeError, match="positions=True"):
        next(off.get_position_minibatches(4))


class _StubRollout:
    """What train() touches of a DeviceRollout, recording how it was built."""
    built = []

    def __init__(self, num_envs, env_offset, global_envs, seed, reward_config, rollout_steps, device, **kw):
        self.kw = kw
        self.buffer = object()
        self.x = torch.zeros(1)
        _StubRollout.built.append(self)

    def reset(self):
        pass

    def collect(self, agent, graph=False):
        pass

    def episodes(self, world):
        return 0, 0, [], []

    def safe_stats(self, world):
        return 0.0, 0

    def close(self):
        pass


class _StubAgent:
    calls = []

    def __init__(self, cfg, device):
        self.config = cfg
        self.network = torch.nn.Linear(1, 1)
        self.autocast_dtype = None

    def train(self):
        pass

    def values_device(self, x):
        return x

    def update(self, buffer, last_values, batch_size=None):
        _StubAgent.calls.append(("update", {}))
        return {k: 0.0 for k in ("policy_loss", "value_loss", "entropy", "total_loss", "approx_kl", "clip_fraction")}

    def distill(self, buffer, **kw):
        from agents.ppo import DISTILL_KEYS

        _StubAgent.calls.append(("distill", kw))
        return {k: 0.0 for k in DISTILL_KEYS}

    def save(self, path):
        pass


def _stub_train(monkeypatch, tmp_path, distill):
    from training import trainer

    monkeypatch.setattr(trainer, "DeviceRollout", _StubRollout)
    monkeypatch.setattr(trainer, "PPOAgent", _StubAgent)
    monkeypatch.setattr(trainer, "broadcast_parameters", lambda agent: None)
    monkeypatch.setattr(trainer, "get_device", lambda verbose=True: torch.device("cpu"))
    _StubRollout.built, _StubAgent.calls = [], []
    cfg = {"training": {"num_envs": 4, "batch_size": 8, "rollout_steps": 2, "total_timesteps": 10 ** 9},
           "logging": {"log_interval": 1, "save_interval": 1000},
           "paths": {"checkpoint_dir": str(tmp_path / "ck"), "log_dir": str(tmp_path / "logs"),
                     "results_dir": str(tmp_path / "res")}}
    if distill is not None:
        cfg["training"]["distill"] = distill
    s = trainer.train(cfg, seed=1, max_updates=3)
    assert s["updates"] == 3
    logs = list((tmp_path / "logs").glob("ppo_*.jsonl"))
    return [json.loads(x) for x in logs[0].read_text().splitlines()]


@pytest.mark.parametrize("distill", [None, {}, {"updates": 0, "tau": 3.0}])
def test_train_without_the_block_stays_on_update(monkeypatch, tmp_path, capsys, distill):
    recs = _stub_train(monkeypatch, tmp_path, distill)
    assert [c[0] for c in _StubAgent.calls] == ["update"] * 3
    assert not _StubRollout.built[0].kw.get("positions", False)
    assert "training.distill" not in capsys.readouterr().out
    assert all("policy_loss" in r and not any(k.startswith("distill") for k in r) for r in recs)


def test_train_with_the_block_distills_first(monkeypatch, tmp_path, capsys):
    from agents.greedy import DEFAULT_WEIGHTS
    from agents.ppo import DISTILL_KEYS

    recs = _stub_train(monkeypatch, tmp_path, {"updates": 2})
    assert [c[0] for c in _StubAgent.calls] == ["distill", "distill", "update"]
    assert _StubAgent.calls[0][1] == dict(batch_size=8, weights=DEFAULT_WEIGHTS, depth=3, tau=50.0, epochs=1)
    assert _StubRollout.built[0].kw["positions"] is True
    assert capsys.readouterr().out.count("training.distill") == 1
    for r in recs[:2]:
        assert set(DISTILL_KEYS) <= set(r) and "policy_loss" not in r
    assert "policy_loss" in recs[2] and not any(k.startswith("distill") for k in recs[2])


def _args(**kw):
    from runtime import lib as L

    a = {k: FAKE for k, _ in L.DistillLossArgs._fields_ if k not in ("bf16", "B", "tau")}
    return L.DistillLossArgs(**{**a, "B": 4, "tau": 50.0, **kw})


_FWD, _BWD = "logits mask_bits q ws cnt stats", "logits mask_bits q grad_loss dlogits"
_FORMS = {"bb_distill_loss_forward": _FWD, "bb_distill_loss_backward": _BWD,
          "bb_distill_loss_fused": _FWD + " grad_loss dlogits"}
_RULE = {"logits": "logits, mask_bits and q are required", "mask_bits": "logits, mask_bits and q are required",
         "q": "logits, mask_bits and q are required", "ws": "ws, cnt and stats are required",
         "cnt": "ws, cnt and stats are required", "stats": "ws, cnt and stats are required",
         "grad_loss": "grad_loss and dlogits are required", "dlogits": "grad_loss and dlogits are required"}
BAD = ([(fn, None, "NULL argument struct") for fn in _FORMS]
       + [(fn, dict(B=-1), "B is negative") for fn in _FORMS]
       + [(fn, dict(tau=t), "tau must be finite and >= 0") for fn in _FORMS
          for t in (-1.0, float("inf"), float("nan"))]
       + [(fn, {k: None}, _RULE[k]) for fn, ks in _FORMS.items() for k in ks.split()])


@pytest.mark.parametrize("fn,kw,msg", BAD, ids=[f"{i}-{c[0]}-{c[2][:12]}" for i, c in enumerate(BAD)])
def test_argument_rules_before_any_hip_call(lib, fn, kw, msg):
    from runtime import lib as L

    a = _args(**kw) if kw is not None else None
    assert getattr(lib, fn)(C.byref(a) if a is not None else None, None) == -1  # BB_ERR_ARG
    assert L.last_error() == f"{fn}: {msg}"


def test_empty_batch_does_nothing_and_struct_layout(lib, tmp_path):
    import os
    import subprocess

    from runtime import lib as L

    for fn in _FORMS:  # B == 0: BB_OK without a launch (the pointers are never read, and there is no device here)
        assert getattr(lib, fn)(C.byref(_args(B=0)), None) == 0
    assert lib.bb_distill_loss_workspace_bytes(-1) == -1
    assert lib.bb_distill_loss_workspace_bytes(259) == 8 * 5 * 65  # 5 fp64 sums per block of 4 rows
    assert lib.bb_distill_loss_forward(C.byref(_args(loss=None, grad_loss=None, dlogits=None, B=0)), None) == 0
    header = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include")
    src = ["#include <stddef.h>\n#include <stdio.h>\n#include \"bbvec.h\"\nint main(void) {",
           'printf("%zu\\n", sizeof(bb_distill_loss_args));']
    want = [C.sizeof(L.DistillLossArgs)]
    for field, _ in L.DistillLossArgs._fields_:
        src.append(f'printf("%zu\\n", offsetof(bb_distill_loss_args, {field}));')
        want.append(getattr(L.DistillLossArgs, field).offset)
    (tmp_path / "sizes.cpp").write_text("\n".join(src) + "\nreturn 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", header, str(tmp_path / "sizes.cpp"), "-o", exe],
                   check=True)
    assert [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()] == want
