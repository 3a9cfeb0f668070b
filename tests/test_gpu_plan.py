"""Full-hand lookahead on the MI355X (plan_kernel in csrc/bb_lookahead.hip: bb_plan_actions / bb_plan_actions_pos).

* Against the chained one-ply reference (tests/_plan_ref.py, which calls no new entry point) at n = 1, 5 and 67
  of the reference set, stateless and handle form, depth 1-3, three weight sets.
* Against the host backend, all four outputs, at n = 1,031 mid-game positions (40 ``bb_rollout`` steps), on fresh
  boards (every list full) and above the kernel's grid cap.
* Depth 1 against the one-ply greedy kernel; NULL optional outputs; a graph replay; the agent replayed through
  the oracle.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _plan_ref as P
from oracle import bb_game as O

pytestmark = pytest.mark.gpu

N_MID = 1031
PLAN_MAX_GRID = 1 << 14  # kPlanMaxGrid of csrc/bb_lookahead.hip
KEYS = ("action", "value", "plan", "leaves")


@pytest.fixture(scope="module")
def ref():
    return R.reference()


def _subset(ref, n):
    """n positions of the set, the crafted ones first (they are its tail), then played ones from the front."""
    crafted = sorted(ref["names"].values())
    return np.array((crafted + [i for i in range(ref["n"]) if i not in crafted])[:n])


def _outputs(n, dev):
    return {"action": torch.full((n,), -7, dtype=torch.int32, device=dev),
            "value": torch.full((n,), 5, dtype=torch.int64, device=dev),
            "plan": torch.full((n, 3), -7, dtype=torch.int32, device=dev),
            "leaves": torch.full((n,), -7, dtype=torch.int32, device=dev)}


def _handle_plan(env, w, depth):
    o = _outputs(env.num_envs, env.device)
    env.plan_actions(o["action"], w, depth, value=o["value"], plan=o["plan"], leaves=o["leaves"])
    return o


def _rolled(n, steps, seed0, dev):
    """n games from seeds seed0 + i after `steps` bb_rollout steps of random legal play (auto-reset on)."""
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(n, [seed0 + i for i in range(n)], device=dev)
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    a0 = torch.zeros(n, dtype=torch.int32, device=dev)
    env.obs(mask_bits=mb)
    env.random_actions(mb, a0, step=0)
    env.rollout(steps, a0, torch.zeros((steps, n), device=dev), torch.zeros((steps, n), dtype=torch.uint8, device=dev))
    env.sync()
    return env


def _host_plan(st, w, depth):
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return K.plan_actions(torch.from_numpy(st["board"].view(np.int64).copy()),
                          torch.from_numpy(st["hand"].view(np.int32).copy()), w, depth,
                          combo=torch.from_numpy(st["combo"].copy()), want_plan=True, want_leaves=True)


def _assert_same(got, want, what):
    for k in KEYS:
        g, x = got[k].cpu(), torch.as_tensor(want[k])
        bad = torch.nonzero((g != x).reshape(g.shape[0], -1).any(dim=1)).flatten()[:4]
        assert bad.numel() == 0, (what, k, bad.tolist(), g[bad].tolist(), x[bad].tolist())


@pytest.mark.parametrize("n", [1, 5, 67])
def test_plan_matches_chained_reference(cuda, ref, n):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    idx = _subset(ref, n)
    board, hand, combo, _ = R.tensors(ref, cuda, idx)
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    before = env.state()
    for depth in (1, 2, 3):
        for wname, w in P.WEIGHT_SETS.items():
            want = {k: v[idx] for k, v in P.reference_plans(depth)[wname].items()}
            got = K.plan_actions(board, hand, w, depth, combo=combo, want_plan=True, want_leaves=True)
            _assert_same(got, want, f"_pos n={n} depth={depth} {wname}")
            _assert_same(_handle_plan(env, w, depth), want, f"handle n={n} depth={depth} {wname}")
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


@pytest.fixture(scope="module")
def mid(cuda):
    env = _rolled(N_MID, 40, 7, cuda)
    yield env, env.state()
    env.close()


def test_mid_game_hip_equals_host_backend(cuda, mid):
    env, st = mid
    for w in (R.DEFAULT_WEIGHTS, P.MIXED):
        host = _host_plan(st, w, 3)
        _assert_same(_handle_plan(env, w, 3), host, "mid-game depth 3")
    slots = P.unused_slots(st["hand"])
    assert {1, 2, 3} <= set(slots.tolist())
    assert int(host["leaves"].max()) > 100_000, int(host["leaves"].max())
    assert bool((host["plan"] == -1).any()) and bool((host["plan"][:, 2] >= 0).any())
    print(f"mid-game: leaves mean {host['leaves'].float().mean():.0f}, max {int(host['leaves'].max())}")


def test_fresh_boards_hip_equals_host_backend(cuda):
    """Empty boards: every anchor of every piece is legal, every list of the kernel is as long as it gets."""
    from runtime.device_env import DeviceEnvBatch

    n = 3
    env = DeviceEnvBatch(n, [7, 8, 9], autoreset=False, device=cuda)
    env.reset()
    st = env.state()
    assert (st["board"] == 0).all()
    host = _host_plan(st, P.MIXED, 3)
    assert int(host["leaves"].min()) > 50_000
    _assert_same(_handle_plan(env, P.MIXED, 3), host, "fresh boards depth 3")
    env.close()


def test_more_positions_than_workgroups(cuda):
    """n = the grid cap + 3: the first three workgroups take a second position.  Depth 2 keeps the host side short."""
    n = PLAN_MAX_GRID + 3
    env = _rolled(n, 25, 1000, cuda)
    host = _host_plan(env.state(), P.MIXED, 2)
    _assert_same(_handle_plan(env, P.MIXED, 2), host, "above the grid cap, depth 2")
    env.close()


def test_depth_one_equals_greedy_kernel(cuda, mid):
    env, _ = mid
    for w in (R.DEFAULT_WEIGHTS, {}, P.MIXED):
        act = torch.zeros(N_MID, dtype=torch.int32, device=cuda)
        val = torch.zeros(N_MID, dtype=torch.int64, device=cuda)
        env.greedy_actions(act, w, value=val)
        got = _handle_plan(env, w, 1)
        assert torch.equal(got["action"], act) and torch.equal(got["value"], val)
        assert bool((got["plan"][:, 0] == act).all()) and bool((got["plan"][:, 1:] == -1).all())


def test_optional_outputs_null_one_at_a_time(cuda, mid):
    env, _ = mid
    full = _handle_plan(env, P.MIXED, 3)
    for skip in ("value", "plan", "leaves", None):
        o = _outputs(N_MID, cuda)
        args = {k: (None if k == skip else o[k]) for k in ("value", "plan", "leaves")}
        env.plan_actions(o["action"], P.MIXED, 3, **args)
        for k in KEYS:
            if k == skip:
                assert bool((o[k] == (5 if k == "value" else -7)).all()), (skip, "written")
            else:
                assert torch.equal(o[k], full[k]), (skip, k)


def test_graph_replay_equals_eager(cuda, mid):
    env, _ = mid
    eager = _handle_plan(env, R.DEFAULT_WEIGHTS, 3)
    o = _outputs(N_MID, cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.plan_actions(o["action"], R.DEFAULT_WEIGHTS, 3, value=o["value"], plan=o["plan"], leaves=o["leaves"])
    for t in o.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(o[k], eager[k]), k


def test_plan_agent_replays_through_oracle(cuda):
    from agents import GreedyAgent, HandPlanAgent
    from evaluation.evaluate import evaluate_agent

    n, seed, cut = 8, 42, 60
    res = evaluate_agent(HandPlanAgent(device=cuda), num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    for ep in range(n):
        env = O.Env(seed=seed + ep)
        obs, info = env.reset(seed=seed + ep)
        term = False
        for t, a in enumerate(res["actions"][ep]):
            assert not term and obs["action_mask"][a] == 1, (ep, t, a)
            obs, _, term, _, info = env.step(a)
        assert term or len(res["actions"][ep]) == cut, ep
        assert res["scores"][ep] == info["score"] and res["lengths"][ep] == len(res["actions"][ep]), ep
    one = evaluate_agent(HandPlanAgent(depth=1, device=cuda), num_episodes=n, seed=seed, max_moves=cut,
                         record_actions=True)
    greedy = evaluate_agent(GreedyAgent(device=cuda), num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    assert one["actions"] == greedy["actions"]
