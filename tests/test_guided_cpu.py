"""Search-guided PPO off the GPU: the fp64 restatement (tests/_guided_ref.py) against finite differences of its own
forward, ``agents.ppo.guided_loss_torch`` against the restatement, the argument rules of the bb_guided_loss entry
points (checked before any HIP call, so they show without a device), the struct layout, the rollout buffer's guided
minibatches and the trainer's ``training.distill.value_coef`` / ``training.guide`` switches on a stub agent.

Tolerances (the project's, tests/test_gpu_ppo_kernels.py and tests/test_gpu_distill_loss.py): loss and statistics
rtol 1e-5 / atol 1e-6, clip_fraction within 2 / B, rows and agreement exact, dvalues rtol 1e-5 / atol 1e-9, dlogits
rtol 1e-4 / atol 1e-5 max|grad|."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _distill_ref as D
import _guided_ref as R
from _guided_ref import BETA, CLIP, CORNERS, EC, VC, check_grads, check_stats

FAKE = 0x10000  # a host integer standing for a device pointer: validation never dereferences it


def test_restatement_gradient_is_its_forwards_derivative():
    """Central finite differences of the restatement's forward in fp64 (B = 5: the five row kinds) against its
    hand-derived gradient, for the logits on M and the values."""
    logits, values, mb, actions, old, adv, ret, q = R.synthetic(5, seed=3)
    x, v = logits.astype(np.float64), values.astype(np.float64)
    coefs = (1.0, VC, 0.05, BETA, 50.0)
    want = R.reference(x, v, mb, actions, old, adv, ret, q, CLIP, coefs, grad_loss=0.75)
    total = lambda xx, vv: 0.75 * R.forward(xx, vv, mb, actions, old, adv, ret, q, CLIP, coefs)[3]  # noqa: E731
    M = D.mask_bool(mb)
    h = 1e-6
    rng = np.random.default_rng(0)
    for i in range(5):
        idx = np.flatnonzero(M[i])
        for a in (idx if idx.size <= 12 else np.unique(np.r_[rng.choice(idx, 10, replace=False), actions[i]])):
            up, dn = x.copy(), x.copy()
            up[i, a] += h
            dn[i, a] -= h
            fd = (total(up, v) - total(dn, v)) / (2 * h)
            assert fd == pytest.approx(want["dlogits"][i, a], rel=1e-5, abs=1e-8), (i, a)
        up, dn = v.copy(), v.copy()
        up[i] += h
        dn[i] -= h
        assert (total(x, up) - total(x, dn)) / (2 * h) == pytest.approx(want["dvalues"][i], rel=1e-6, abs=1e-9)
    assert not want["dlogits"][0].any() and want["dvalues"][0] == 0  # row 0: empty M
    assert want["dlogits"][1].any()  # row 1: M without S still has its PPO gradient


def _torch_call(rows, coefs, g, q_none=False):
    from agents.ppo import guided_loss_torch

    logits, values, mb, actions, old, adv, ret, q = rows
    x = torch.from_numpy(logits).requires_grad_(True)
    v = torch.from_numpy(values).requires_grad_(True)
    t = [torch.from_numpy(a) for a in (mb, actions, old, adv, ret)]
    loss, stats = guided_loss_torch(x, v, *t, None if q_none else torch.from_numpy(q), CLIP, coefs)
    loss.backward(torch.tensor(g))
    return loss, stats, x.grad.numpy().astype(np.float64), v.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("corner", list(CORNERS))
@pytest.mark.parametrize("tau", [0.0, 1.0, 50.0, 1e4])
@pytest.mark.parametrize("density", ["one", "tenth", "all"])
def test_torch_loss_matches_fp64_restatement(density, tau, corner):
    B = 37
    rows = R.synthetic(B, seed=21, density=density)
    coefs = (*CORNERS[corner], tau)
    want = R.reference(*rows, CLIP, coefs, grad_loss=0.75)
    loss, stats, dl, dv = _torch_call(rows, coefs, 0.75)
    assert stats.shape == (12,) and loss.item() == stats[3].item()
    check_stats(stats.double().numpy(), want["stats"], B)
    check_grads(dl, dv, want, rows[2])


def test_torch_loss_without_q():
    rows = R.synthetic(37, seed=22)
    coefs = (1.0, VC, EC, 0.0, 50.0)
    want = R.reference(*rows[:7], None, CLIP, coefs)
    _, stats, dl, dv = _torch_call(rows, coefs, 1.0, q_none=True)
    assert not stats[6:].any()
    check_stats(stats.double().numpy(), want["stats"], 37)
    check_grads(dl, dv, want, rows[2])


@pytest.mark.parametrize("tau", [0.0, 50.0])
def test_torch_loss_is_ppo_plus_beta_distill(tau):
    """policy_coef = 1: the PPO loss on the expanded mask plus beta times the distillation loss (no empty-M row:
    the PPO chain has no rule for one)."""
    from agents.ppo import PPOConfig, distill_loss_torch, guided_loss_torch, ppo_loss_torch

    logits, values, mb, actions, old, adv, ret, q = R.synthetic(37, seed=23, kinds=False)
    t = {k: torch.from_numpy(a) for k, a in dict(mb=mb, a=actions, old=old, adv=adv, ret=ret, q=q).items()}
    cfg = PPOConfig(clip_epsilon=CLIP, value_coef=VC, entropy_coef=EC)

    def grads(fn):
        x, v = torch.from_numpy(logits).requires_grad_(True), torch.from_numpy(values).requires_grad_(True)
        loss, stats = fn(x, v)
        loss.backward()
        return loss.detach(), stats, x.grad, v.grad

    mask = torch.from_numpy(D.mask_bool(mb)).float()
    gl, gs, gx, gv = grads(lambda x, v: guided_loss_torch(x, v, t["mb"], t["a"], t["old"], t["adv"], t["ret"],
                                                          t["q"], CLIP, (1.0, VC, EC, BETA, tau)))
    kept = []

    def pair(x, v):
        pl, ps = ppo_loss_torch(x, v, mask, t["a"], t["old"], t["adv"], t["ret"], cfg)
        dl, ds = distill_loss_torch(x, t["mb"], t["q"], tau)
        kept.append((ps, ds))
        return pl + BETA * dl, None

    pl, _, px, pv = grads(pair)
    ps, ds = kept[0]
    torch.testing.assert_close(gl, pl, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(gs[[0, 1, 2, 4, 5]], ps[[0, 1, 2, 4, 5]], rtol=1e-6, atol=1e-7)
    assert torch.equal(gs[6:], ds)
    torch.testing.assert_close(gx, px, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(gv, pv, rtol=1e-6, atol=1e-10)


# ---------------------------------------------------------------------------------------------- the entry points
def _args(**kw):
    from runtime import lib as L

    scalars = dict(bf16=0, B=4, clip=CLIP, policy_coef=1.0, value_coef=VC, entropy_coef=EC, distill_coef=BETA,
                   tau=50.0, coefs_dev=None)
    a = {k: FAKE for k, _ in L.GuidedLossArgs._fields_ if k not in scalars}
    return L.GuidedLossArgs(**{**a, **scalars, **kw})


_ROWS = "logits values mask_bits actions old_logp adv ret"
_FWD, _BWD = "ws cnt stats", "grad_loss dlogits dvalues"
_FORMS = {"bb_guided_loss_forward": _FWD, "bb_guided_loss_backward": _BWD, "bb_guided_loss_fused": _FWD + " " + _BWD}
_RULE = {**{k: "logits, values, mask_bits, actions, old_logp, adv and ret are required" for k in _ROWS.split()},
         **{k: "ws, cnt and stats are required" for k in _FWD.split()},
         **{k: "grad_loss, dlogits and dvalues are required" for k in _BWD.split()}}
_COEFS = ("policy_coef", "value_coef", "entropy_coef", "distill_coef")
_NOT_OK = (-1.0, float("inf"), float("nan"))
BAD = ([(fn, None, "NULL argument struct") for fn in _FORMS]
       + [(fn, dict(B=-1), "B is negative") for fn in _FORMS]
       + [(fn, dict(tau=t), "tau must be finite and >= 0") for fn in _FORMS for t in _NOT_OK]
       + [(fn, dict(clip=t), "clip must be finite and >= 0") for fn in _FORMS for t in _NOT_OK]
       + [("bb_guided_loss_fused", {k: t}, "coefficients must be finite and >= 0") for k in _COEFS for t in _NOT_OK]
       + [(fn, dict(q=None), "q is required when distill_coef != 0") for fn in _FORMS]
       + [(fn, dict(q=None, distill_coef=0.0, coefs_dev=FAKE), "q is required with coefs_dev") for fn in _FORMS]
       + [(fn, {k: None}, _RULE[k]) for fn, ks in _FORMS.items() for k in (_ROWS + " " + ks).split()])


@pytest.mark.parametrize("fn,kw,msg", BAD, ids=[f"{i}-{c[0][16:]}-{c[2][:14]}" for i, c in enumerate(BAD)])
def test_argument_rules_before_any_hip_call(lib, fn, kw, msg):
    from runtime import lib as L

    a = _args(**kw) if kw is not None else None
    assert getattr(lib, fn)(C.byref(a) if a is not None else None, None) == -1  # BB_ERR_ARG
    assert L.last_error() == f"{fn}: {msg}"


def test_empty_batch_workspace_and_struct_layout(lib, tmp_path):
    import os
    import subprocess

    from runtime import kernels as K
    from runtime import lib as L

    for fn in _FORMS:  # B == 0: BB_OK without a launch (the pointers are never read, and there is no device here)
        assert getattr(lib, fn)(C.byref(_args(B=0)), None) == 0
    # q may be NULL when distill_coef == 0 and there is no coefs_dev; loss is optional
    assert lib.bb_guided_loss_forward(C.byref(_args(B=0, q=None, distill_coef=0.0, loss=None)), None) == 0
    assert lib.bb_guided_loss_workspace_bytes(-1) == -1
    assert lib.bb_guided_loss_workspace_bytes(0) == 8 * 10
    assert lib.bb_guided_loss_workspace_bytes(259) == 8 * 10 * 65  # 10 fp64 sums per block of 4 rows
    assert lib.bb_guided_loss_workspace_bytes(1 << 20) == 8 * 10 * 4096  # at most 4,096 blocks
    assert K.GUIDED_STATS == R.STATS and len(K.GUIDED_STATS) == 12
    header = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include")
    src = ["#include <stddef.h>\n#include <stdio.h>\n#include \"bbvec.h\"\nint main(void) {",
           'printf("%zu\\n", sizeof(bb_guided_loss_args));']
    want = [C.sizeof(L.GuidedLossArgs)]
    for field, _ in L.GuidedLossArgs._fields_:
        src.append(f'printf("%zu\\n", offsetof(bb_guided_loss_args, {field}));')
        want.append(getattr(L.GuidedLossArgs, field).offset)
    (tmp_path / "sizes.cpp").write_text("\n".join(src) + "\nreturn 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", header, str(tmp_path / "sizes.cpp"), "-o", exe],
                   check=True)
    assert [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()] == want


# ------------------------------------------------------------------------------------------- the rollout buffer
def test_guided_minibatches_are_the_ppo_and_position_rows(monkeypatch):
    """Under the same generator get_guided_minibatches yields the rows of get_minibatches (mask words in place of
    the f32 mask) and of get_position_minibatches.  bb_gather_obs is a HIP kernel: here a stand-in that expands the
    selected rows with torch ops, so what is compared is the row selection."""
    from agents.ppo import PackedRolloutBuffer
    from runtime import kernels as K

    def gather(board, hand, mask_bits, index, want_x=True, want_mask=True, out_x=None, out_mask=None):
        x = (board[index].double() * 1e-18 + hand[index]).float().reshape(-1, 1, 1, 1).expand(-1, 4, 8, 8)
        return (x if want_x else None), (K.mask_bits_to_bool(mask_bits[index]).float() if want_mask else None)

    monkeypatch.setattr(K, "gather_obs", gather)
    T, N = 6, 8
    buf = PackedRolloutBuffer(T, N, torch.device("cpu"), positions=True)
    g = torch.Generator().manual_seed(5)
    buf.board.copy_(torch.randint(-2 ** 62, 2 ** 62, (T, N), generator=g))
    buf.hand.copy_(torch.randint(0, 2 ** 20, (T, N), generator=g, dtype=torch.int32))
    buf.combo.copy_(torch.randint(0, 9, (T, N), generator=g, dtype=torch.int32))
    buf.mask_bits.copy_(torch.randint(-2 ** 62, 2 ** 62, (T, N, 3), generator=g))
    buf.actions.copy_(torch.randint(0, 192, (T, N), generator=g))
    for t in (buf.log_probs, buf.advantages, buf.returns):
        t.copy_(torch.randn(T, N, generator=g))
    gen = lambda: torch.Generator().manual_seed(9)  # noqa: E731
    guided = list(buf.get_guided_minibatches(20, generator=gen()))
    ppo = list(buf.get_minibatches(20, generator=gen()))
    pos = list(buf.get_position_minibatches(20, generator=gen()))
    assert [b[0].shape[0] for b in guided] == [20, 20, 8]
    for gb, pb, qb in zip(guided, ppo, pos):
        assert len(gb) == 9
        assert torch.equal(gb[0], pb[0]) and torch.equal(gb[0], qb[0])
        assert torch.equal(K.mask_bits_to_bool(gb[1]).float(), pb[1]) and torch.equal(gb[1], qb[1])
        for a, b in zip(gb[2:6], pb[2:6]):
            assert torch.equal(a, b)
        for a, b in zip(gb[6:9], qb[2:5]):
            assert torch.equal(a, b)
    # out(B): the yielded tensors are the buffers handed in, holding the same rows
    keep = {}

    def out(b):
        if b not in keep:
            keep[b] = tuple(torch.empty_like(t) for t in [x for x in guided if x[0].shape[0] == b][0])
        return keep[b]

    def gather_into(board, hand, mask_bits, index, want_x=True, want_mask=True, out_x=None, out_mask=None):
        out_x.copy_(gather(board, hand, mask_bits, index, want_mask=False)[0])
        return out_x, None

    monkeypatch.setattr(K, "gather_obs", gather_into)
    for gb, ob in zip(guided, buf.get_guided_minibatches(20, generator=gen(), out=out)):
        assert all(o is k for o, k in zip(ob, keep[ob[0].shape[0]]))
        assert all(torch.equal(a, b) for a, b in zip(gb, ob))
    with pytest.raises(RuntimeError, match="positions=True"):
        next(PackedRolloutBuffer(T, N, torch.device("cpu")).get_guided_minibatches(4))


# --------------------------------------------------------------------------------------------------- the trainer
PPO_KEYS = ("policy_loss", "value_loss", "entropy", "total_loss", "approx_kl", "clip_fraction")


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
        _StubAgent.calls.append(("update", dict(batch_size=batch_size)))
        return {k: 0.0 for k in PPO_KEYS}

    def distill(self, buffer, **kw):
        from agents.ppo import DISTILL_KEYS

        _StubAgent.calls.append(("distill", kw))
        return {k: 0.0 for k in DISTILL_KEYS}

    def update_guided(self, buffer, last_values, **kw):
        from agents.ppo import DISTILL_KEYS

        _StubAgent.calls.append(("update_guided", kw))
        return {k: 0.0 for k in PPO_KEYS + DISTILL_KEYS}

    def save(self, path):
        pass


def _stub_train(monkeypatch, tmp_path, updates, **training):
    from training import trainer

    monkeypatch.setattr(trainer, "DeviceRollout", _StubRollout)
    monkeypatch.setattr(trainer, "PPOAgent", _StubAgent)
    monkeypatch.setattr(trainer, "broadcast_parameters", lambda agent: None)
    monkeypatch.setattr(trainer, "get_device", lambda verbose=True: torch.device("cpu"))
    _StubRollout.built, _StubAgent.calls = [], []
    cfg = {"ppo": {"value_coef": 0.25, "entropy_coef": 0.02},
           "training": {"num_envs": 4, "batch_size": 8, "rollout_steps": 2, "total_timesteps": 10 ** 9, **training},
           "logging": {"log_interval": 1, "save_interval": 1000},
           "paths": {"checkpoint_dir": str(tmp_path / "ck"), "log_dir": str(tmp_path / "logs"),
                     "results_dir": str(tmp_path / "res")}}
    assert trainer.train(cfg, seed=1, max_updates=updates)["updates"] == updates
    logs = list((tmp_path / "logs").glob("ppo_*.jsonl"))
    return [json.loads(x) for x in logs[0].read_text().splitlines()]


@pytest.mark.parametrize("training", [{}, {"guide": {}}, {"guide": {"beta": 0, "beta_final": 0.0, "tau": 3.0}},
                                      {"distill": {"updates": 2}}, {"distill": {"updates": 2, "value_coef": 0}},
                                      {"distill": {"value_coef": 0.5}}],
                         ids=["none", "empty-guide", "zero-betas", "distill", "distill-vc0", "vc-without-updates"])
def test_train_without_the_new_keys_makes_todays_calls(monkeypatch, tmp_path, capsys, training):
    from agents.greedy import DEFAULT_WEIGHTS

    recs = _stub_train(monkeypatch, tmp_path, 3, **training)
    n = int(training.get("distill", {}).get("updates", 0))
    want = [("distill", dict(batch_size=8, weights=DEFAULT_WEIGHTS, depth=3, tau=50.0, epochs=1))] * n
    want += [("update", dict(batch_size=8))] * (3 - n)
    assert _StubAgent.calls == want
    assert bool(_StubRollout.built[0].kw.get("positions", False)) == (n > 0)
    out = capsys.readouterr().out
    assert "training.guide" not in out and "value_coef" not in out
    assert not any("guide_beta" in r for r in recs)


def test_train_distills_with_the_critic(monkeypatch, tmp_path, capsys):
    from agents.greedy import DEFAULT_WEIGHTS
    from agents.ppo import DISTILL_KEYS

    recs = _stub_train(monkeypatch, tmp_path, 3,
                       distill={"updates": 2, "value_coef": 0.5, "epochs": 2, "depth": 2, "tau": 7.0})
    assert [c[0] for c in _StubAgent.calls] == ["update_guided", "update_guided", "update"]
    assert _StubAgent.calls[0][1] == dict(weights=DEFAULT_WEIGHTS, depth=2, tau=7.0, coefs=(0.0, 0.5, 0.0, 1.0),
                                          batch_size=8, epochs=2)
    assert _StubRollout.built[0].kw["positions"] is True
    out = capsys.readouterr().out
    assert out.count("training.distill") == 1 and out.count("value_coef 0.5") == 1
    for r in recs[:2]:
        assert set(DISTILL_KEYS) <= set(r) and set(PPO_KEYS) <= set(r) and "guide_beta" not in r
    assert "policy_loss" in recs[2] and not any(k.startswith("distill") for k in recs[2])


def test_train_guide_follows_the_linear_schedule(monkeypatch, tmp_path, capsys):
    from agents.ppo import DISTILL_KEYS

    w = {"lines": 100, "score": 0, "holes": -30, "filled": -2, "centre": 0, "mobility": 1, "dead": -100000,
         "refill": 0}
    recs = _stub_train(monkeypatch, tmp_path, 8, distill={"updates": 1, "depth": 2, "tau": 9.0, "weights": w},
                       guide={"beta": 1.0, "beta_final": 0.25, "decay_updates": 4})
    assert [c[0] for c in _StubAgent.calls] == ["distill"] + ["update_guided"] * 7
    betas = [c[1]["coefs"][3] for c in _StubAgent.calls[1:]]
    assert betas == pytest.approx([1.0, 0.8125, 0.625, 0.4375, 0.25, 0.25, 0.25])  # counted from the first PPO one
    for c in _StubAgent.calls[1:]:  # PPOConfig's coefficients, the distill block's search, num_epochs passes
        assert c[1]["coefs"][:3] == (1.0, 0.25, 0.02)
        assert c[1] == dict(coefs=c[1]["coefs"], batch_size=8, weights=w, depth=2, tau=9.0)
    assert _StubRollout.built[0].kw["positions"] is True
    assert capsys.readouterr().out.count("training.guide") == 1
    assert "guide_beta" not in recs[0]
    assert [r["guide_beta"] for r in recs[1:]] == pytest.approx(betas)
    assert all(set(DISTILL_KEYS) <= set(r) and set(PPO_KEYS) <= set(r) for r in recs[1:])


def test_train_guide_decays_to_plain_ppo_and_takes_its_own_search(monkeypatch, tmp_path):
    recs = _stub_train(monkeypatch, tmp_path, 4, guide={"beta": 0.5, "decay_updates": 2, "depth": 1, "tau": 3.0})
    assert [c[0] for c in _StubAgent.calls] == ["update_guided", "update_guided", "update", "update"]
    assert [c[1]["coefs"][3] for c in _StubAgent.calls[:2]] == [0.5, 0.25]
    assert _StubAgent.calls[0][1]["depth"] == 1 and _StubAgent.calls[0][1]["tau"] == 3.0
    assert _StubRollout.built[0].kw["positions"] is True  # the block implies stored positions
    assert "guide_beta" not in recs[2] and not any(k.startswith("distill") for k in recs[3])
    _stub_train(monkeypatch, tmp_path / "b", 3, guide={"beta": 0.5})  # no decay_updates: it stays at beta
    assert [c[1]["coefs"][3] for c in _StubAgent.calls] == [0.5] * 3
