"""One-ply lookahead on the MI355X (csrc/bb_lookahead.hip: bb_afterstates / bb_greedy_actions).

* Against the unmodified oracle (tests/_afterstates_ref.py: ``copy.deepcopy(env).step(a)`` for every action, the
  position set of played and crafted positions) at n = 1, 5 and 67 -- a ragged tail, more than one workgroup --
  through the stateless form and the handle form (no auto-reset), every output of every action, fp64 reward
  with ``==``.
* Against the host backend, bit for bit, at n = 4,099 positions reached by 40 ``bb_rollout`` steps.
* The fused greedy kernel against a torch arg-max over the dense kernel's own outputs at n = 4,099.
* Optional outputs NULL one at a time; both launches captured in a graph replay bit-equal to eager.
* A short greedy evaluation replayed through the oracle.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
from oracle import bb_game as O

pytestmark = pytest.mark.gpu

MIXED = {"lines": -7, "score": 3, "holes": -1, "filled": 1, "centre": 5, "mobility": -2, "dead": 50, "refill": 11}
N_BIG = 4099


@pytest.fixture(scope="module")
def ref():
    return R.reference()


def _subset(ref, n):
    """n positions of the set, the crafted ones first (they are its tail), then played ones from the front."""
    crafted = sorted(ref["names"].values())
    idx = (crafted + [i for i in range(ref["n"]) if i not in crafted])[:n]
    return np.array(idx)


@pytest.mark.parametrize("n", [1, 5, 67])
def test_afterstates_match_oracle(cuda, ref, n):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    idx = _subset(ref, n)
    board, hand, combo, prev = R.tensors(ref, cuda, idx)
    R.check_dense(ref, K.afterstates(board, hand, combo, prev), idx, what=f"_pos n={n}")
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    before = env.state()
    R.check_dense(ref, env.afterstates(), idx, what=f"handle n={n}")
    for w in (R.DEFAULT_WEIGHTS, {}, MIXED):
        want_a, want_v = R.expected_greedy(ref, w)
        act = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        val = torch.zeros(n, dtype=torch.int64, device=cuda)
        env.greedy_actions(act, w, value=val)
        assert np.array_equal(act.cpu().numpy(), want_a[idx]) and np.array_equal(val.cpu().numpy(), want_v[idx])
        a2, v2 = K.greedy_actions(board, hand, w, combo=combo)
        assert torch.equal(a2, act) and torch.equal(v2, val)
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


@pytest.fixture(scope="module")
def played(cuda):
    """4,099 positions: games from seeds 7 + i after 40 bb_rollout steps; (device env, host-side state)."""
    from runtime.device_env import DeviceEnvBatch

    n, T = N_BIG, 40
    env = DeviceEnvBatch(n, [7 + i for i in range(n)], device=cuda)
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64, device=cuda)
    a0 = torch.zeros(n, dtype=torch.int32, device=cuda)
    env.obs(mask_bits=mb)
    env.random_actions(mb, a0, step=0)
    env.rollout(T, a0, torch.zeros((T, n), device=cuda), torch.zeros((T, n), dtype=torch.uint8, device=cuda))
    env.sync()
    yield env, env.state()
    env.close()


def _state_tensors(st, dev):
    prev = st["prev_holes"].astype(np.uint16) | (st["prev_center"].astype(np.uint16) << 8)
    return (torch.from_numpy(st["board"].view(np.int64).copy()).to(dev),
            torch.from_numpy(st["hand"].view(np.int32).copy()).to(dev),
            torch.from_numpy(st["combo"].copy()).to(dev), torch.from_numpy(prev.view(np.int16).copy()).to(dev))


def test_hip_equals_host_backend(cuda, played):
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    env, st = played
    hip = env.afterstates()
    hip_pos = K.afterstates(*_state_tensors(st, cuda))
    host = K.afterstates(*_state_tensors(st, torch.device("cpu")))
    aux = K.unpack_aux(host["aux"])
    # auto-reset envs are never left game-over: every position has a legal action, so nothing compares vacuously
    assert aux["legal"].any(dim=1).all() and aux["refill"].any() and (aux["lines"] > 0).any()
    for k in host:
        # bit patterns: the fp64 rewards through their int64 view
        assert torch.equal(hip[k].cpu().view(torch.int64 if k == "reward" else hip[k].dtype),
                           host[k].view(torch.int64 if k == "reward" else host[k].dtype)), k
        assert torch.equal(hip_pos[k], hip[k]), k
    board, hand, combo, _ = _state_tensors(st, torch.device("cpu"))
    for w in (R.DEFAULT_WEIGHTS, MIXED):
        ha, hv = K.greedy_actions(board, hand, w, combo=combo)
        act = torch.zeros(N_BIG, dtype=torch.int32, device=cuda)
        val = torch.zeros(N_BIG, dtype=torch.int64, device=cuda)
        env.greedy_actions(act, w, value=val)
        assert torch.equal(act.cpu(), ha) and torch.equal(val.cpu(), hv)


def test_more_positions_than_workgroups(cuda):
    """Above 32,768 positions (kLookMaxGrid) the workgroups stride over the positions: n = 32,771 makes the
    first three workgroups take a second position.  HIP against the host backend, bit for bit."""
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    n, T = 32768 + 3, 25
    env = DeviceEnvBatch(n, [1000 + i for i in range(n)], device=cuda)
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64, device=cuda)
    a0 = torch.zeros(n, dtype=torch.int32, device=cuda)
    env.obs(mask_bits=mb)
    env.random_actions(mb, a0, step=0)
    env.rollout(T, a0, torch.zeros((T, n), device=cuda), torch.zeros((T, n), dtype=torch.uint8, device=cuda))
    env.sync()
    st = env.state()
    hip = env.afterstates()
    host = K.afterstates(*_state_tensors(st, torch.device("cpu")))
    for k in host:
        same = hip[k].cpu().view(torch.int64 if k == "reward" else hip[k].dtype) == \
            host[k].view(torch.int64 if k == "reward" else host[k].dtype)
        assert bool(same.all()), (k, torch.nonzero(~same.all(dim=1))[:4].tolist())
    board, hand, combo, _ = _state_tensors(st, torch.device("cpu"))
    ha, hv = K.greedy_actions(board, hand, MIXED, combo=combo)
    act = torch.zeros(n, dtype=torch.int32, device=cuda)
    val = torch.zeros(n, dtype=torch.int64, device=cuda)
    env.greedy_actions(act, MIXED, value=val)
    assert torch.equal(act.cpu(), ha) and torch.equal(val.cpu(), hv)
    env.close()


@pytest.mark.parametrize("wname", ["default", "zero", "mixed"])
def test_greedy_equals_argmax_of_dense_outputs(cuda, played, wname):
    from runtime import kernels as K

    env, _ = played
    w = {"default": R.DEFAULT_WEIGHTS, "zero": {}, "mixed": MIXED}[wname]
    out = env.afterstates()
    f = K.unpack_aux(out["aux"])
    f["score"] = out["score_gained"].long()
    f["filled"] = sum((out["board"] >> s) & 1 for s in range(64))  # popcount; >> is arithmetic, & 1 takes the bit
    v = sum(int(w.get(k, 0)) * f[k].long() for k in R.FIELDS)
    v = torch.where(f["legal"], v, torch.full_like(v, R.INT64_MIN))
    best = v.max(dim=1).values
    first = (v == best[:, None]).long().argmax(dim=1)  # the lowest action among the maxima
    first = torch.where(f["legal"].any(dim=1), first, torch.zeros_like(first))
    act = torch.zeros(N_BIG, dtype=torch.int32, device=cuda)
    val = torch.zeros(N_BIG, dtype=torch.int64, device=cuda)
    env.greedy_actions(act, w, value=val)
    assert torch.equal(act.long(), first) and torch.equal(val, best)


def test_optional_outputs_null_one_at_a_time(cuda, played):
    from runtime import kernels as K

    env, _ = played
    full = env.afterstates()
    keys = ("board", "reward", "score_gained", "aux")
    for skip in keys:
        part = env.afterstates(out=K.afterstate_outputs(N_BIG, cuda, want=tuple(k for k in keys if k != skip)))
        assert skip not in part
        for k in part:
            assert torch.equal(part[k], full[k]), (skip, k)
    act = torch.zeros(N_BIG, dtype=torch.int32, device=cuda)
    ref_act = torch.zeros(N_BIG, dtype=torch.int32, device=cuda)
    env.greedy_actions(ref_act, MIXED, value=torch.zeros(N_BIG, dtype=torch.int64, device=cuda))
    env.greedy_actions(act, MIXED)  # d_value NULL
    assert torch.equal(act, ref_act)


def test_graph_replay_equals_eager(cuda, played):
    from runtime import kernels as K

    env, _ = played
    eager = env.afterstates()
    e_act = torch.zeros(N_BIG, dtype=torch.int32, device=cuda)
    e_val = torch.zeros(N_BIG, dtype=torch.int64, device=cuda)
    env.greedy_actions(e_act, R.DEFAULT_WEIGHTS, value=e_val)
    out = K.afterstate_outputs(N_BIG, cuda)
    act = torch.zeros(N_BIG, dtype=torch.int32, device=cuda)
    val = torch.zeros(N_BIG, dtype=torch.int64, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.afterstates(out=out)
        env.greedy_actions(act, R.DEFAULT_WEIGHTS, value=val)
    for t in list(out.values()) + [act, val]:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(out[k].view(torch.int64 if k == "reward" else out[k].dtype),
                           eager[k].view(torch.int64 if k == "reward" else eager[k].dtype)), k
    assert torch.equal(act, e_act) and torch.equal(val, e_val)


def test_greedy_evaluation_replays_through_oracle(cuda):
    from agents import GreedyAgent
    from evaluation.evaluate import evaluate_agent

    n, seed, cut = 8, 42, 100
    res = evaluate_agent(GreedyAgent(device=cuda), num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    for ep in range(n):
        env = O.Env(seed=seed + ep)
        obs, info = env.reset(seed=seed + ep)
        term = False
        for t, a in enumerate(res["actions"][ep]):
            assert not term and obs["action_mask"][a] == 1, (ep, t, a)
            obs, _, term, _, info = env.step(a)
        assert term or len(res["actions"][ep]) == cut, ep
        assert res["scores"][ep] == info["score"] and res["lengths"][ep] == len(res["actions"][ep]), ep
