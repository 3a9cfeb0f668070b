"""Per-action full-hand values and the hand-safe mask on the MI355X (plan_values_kernel in csrc/bb_lookahead.hip:
bb_plan_values / bb_plan_values_pos).

* A graph capture of the process's first bb_plan_values launch (this test comes first in the file), replayed on
  changed position columns.
* Against the reference of tests/_plan_values_ref.py (which calls no new entry point) at n = 1, 5 and 67 of the
  reference set, stateless and handle form, depth 1-3, three weight sets.
* Against the host backend, all four outputs, at the 1,031 mid-game positions of tests/test_gpu_plan.py and on
  fresh boards at depth 3, and above the kernel's grid cap at depth 2, where a workgroup takes a second position
  and the barrier at the end of a position matters.
* Consistency with bb_plan_actions; NULL-output combinations; hand-safe random play replayed through the oracle.
"""
import itertools

import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _plan_ref as P
import _plan_values_ref as V
from oracle import bb_game as O
from test_gpu_plan import N_MID, PLAN_MAX_GRID, _rolled, _subset

pytestmark = pytest.mark.gpu

KEYS = ("q", "rest", "leaves", "safe")


@pytest.fixture(scope="module")
def ref():
    return R.reference()


def _outputs(n, dev, keys=KEYS):
    from runtime import kernels as K

    return {k: torch.full_like(v, -7) for k, v in K.plan_value_outputs(n, dev, keys).items()}


def _host_values(st, w, depth):
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return K.plan_values(torch.from_numpy(st["board"].view(np.int64).copy()),
                         torch.from_numpy(st["hand"].view(np.int32).copy()), w, depth,
                         combo=torch.from_numpy(st["combo"].copy()))


def _assert_same(got, want, what):
    for k in KEYS:
        g, x = got[k].cpu(), want[k].cpu()
        bad = torch.nonzero(g != x)[:4]
        assert bad.numel() == 0, (what, k, bad.tolist(), [int(g[tuple(b)]) for b in bad], [int(x[tuple(b)]) for b in bad])


def test_graph_capture_of_the_first_call_and_replays(cuda, ref):
    """No eager bb_plan_values launch precedes the capture in this file.  The graph is replayed three times, the
    position columns rewritten in place before the second and third."""
    from runtime import kernels as K

    n = 23
    sets = [np.arange(k, k + n) for k in (0, 30, 60)]
    board, hand, combo, _ = R.tensors(ref, cuda, sets[0])
    o = _outputs(n, cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.plan_values(board, hand, P.MIXED, 3, combo=combo, out=o)
    for idx in sets:
        b, h, c, _ = R.tensors(ref, cuda, idx)
        board.copy_(b), hand.copy_(h), combo.copy_(c)
        for t in o.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        V.check(o, V.reference_values(3), "mixed", idx, what=f"graph replay on positions {idx[0]}..")
        _assert_same(o, K.plan_values(b, h, P.MIXED, 3, combo=c), "graph replay against eager")


@pytest.mark.parametrize("n", [1, 5, 67])
def test_values_match_reference(cuda, ref, n):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    idx = _subset(ref, n)
    board, hand, combo, _ = R.tensors(ref, cuda, idx)
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    before = env.state()
    for depth in (1, 2, 3):
        want = V.reference_values(depth)
        for wname, w in P.WEIGHT_SETS.items():
            V.check(K.plan_values(board, hand, w, depth, combo=combo), want, wname, idx, f"_pos n={n} depth={depth}")
            V.check(env.plan_values(w, depth, out=_outputs(n, cuda)), want, wname, idx, f"handle n={n} depth={depth}")
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
    host = _host_values(st, P.MIXED, 3)
    _assert_same(env.plan_values(P.MIXED, 3, out=_outputs(N_MID, cuda)), host, "mid-game depth 3")
    legal = host["q"] != R.INT64_MIN
    safe = torch.from_numpy(V.safe_bool(host["safe"].numpy()))
    assert {1, 2, 3} <= set(P.unused_slots(st["hand"]).tolist())
    assert int(host["leaves"].sum(dim=1).max()) > 100_000 and bool((legal & ~safe).any())
    assert bool((host["rest"] == 0xFFFF).any()) and bool(((host["rest"] >> 8) != 0xFF)[legal].any())
    print(f"mid-game: {int(legal.sum())} legal actions, {int((legal & ~safe).sum())} unsafe")


def test_fresh_boards_hip_equals_host_backend(cuda):
    """Empty boards: every anchor of every piece is legal, the record list is as long as it gets."""
    from runtime.device_env import DeviceEnvBatch

    n = 3
    env = DeviceEnvBatch(n, [7, 8, 9], autoreset=False, device=cuda)
    env.reset()
    st = env.state()
    assert (st["board"] == 0).all()
    host = _host_values(st, P.MIXED, 3)
    assert int(host["leaves"].sum(dim=1).min()) > 50_000
    _assert_same(env.plan_values(P.MIXED, 3, out=_outputs(n, cuda)), host, "fresh boards depth 3")
    env.close()


def test_more_positions_than_workgroups(cuda):
    """n = the grid cap + 3 = 16,387: the first three workgroups take a second position, whose ply-1 lanes rewrite
    the staging arrays the first position's rows were stored from.  Every game has a seed of its own, so the two
    positions of such a workgroup differ in their legal sets."""
    n = PLAN_MAX_GRID + 3
    assert n == 16387
    env = _rolled(n, 25, 1000, cuda)
    host = _host_values(env.state(), P.MIXED, 2)
    legal = host["q"] != R.INT64_MIN
    for i in range(3):
        assert not torch.equal(legal[i], legal[i + PLAN_MAX_GRID]), i
    assert bool((legal[1:] != legal[:-1]).any(dim=1).float().mean() > 0.9)  # neighbours differ too
    _assert_same(env.plan_values(P.MIXED, 2, out=_outputs(n, cuda)), host, "above the grid cap, depth 2")
    env.close()


def test_consistent_with_plan_actions(cuda, mid):
    from runtime import kernels as K

    env, _ = mid
    for depth, w in ((3, P.MIXED), (3, R.DEFAULT_WEIGHTS), (2, P.MIXED), (1, P.MIXED)):
        got = env.plan_values(w, depth)
        act = torch.zeros(N_MID, dtype=torch.int32, device=cuda)
        val = torch.zeros(N_MID, dtype=torch.int64, device=cuda)
        plan = torch.zeros((N_MID, 3), dtype=torch.int32, device=cuda)
        leaves = torch.zeros(N_MID, dtype=torch.int32, device=cuda)
        env.plan_actions(act, w, depth, value=val, plan=plan, leaves=leaves)
        best = got["q"].max(dim=1).values
        assert torch.equal(best, val), depth
        playable = leaves > 0
        first = (got["q"] == best[:, None]).int().argmax(dim=1).int()
        assert torch.equal(first[playable], act[playable]), depth
        a2, a3 = K.unpack_rest(got["rest"][torch.arange(N_MID, device=cuda), act.long()])
        assert torch.equal(a2[playable], plan[playable, 1]) and torch.equal(a3[playable], plan[playable, 2]), depth
        assert torch.equal(got["leaves"].sum(dim=1).int(), leaves), depth


def test_null_output_combinations(cuda, mid):
    env, _ = mid
    full = env.plan_values(P.MIXED, 3)
    for r in (1, 2, 3):
        for keys in itertools.combinations(KEYS, r):
            o = _outputs(N_MID, cuda)
            env.plan_values(P.MIXED, 3, out={k: o[k] for k in keys})
            for k in KEYS:
                if k in keys:
                    assert torch.equal(o[k], full[k]), (keys, k)
                else:
                    assert bool((o[k] == -7).all()), (keys, k, "written")
    safe = torch.zeros((N_MID, 3), dtype=torch.int64, device=cuda)
    assert torch.equal(env.safe_mask(safe, depth=2), full["safe"])  # the same set one ply shallower


def _replay_never_ends_mid_hand(res, n, seed, cut):
    for ep in range(n):
        env = O.Env(seed=seed + ep)
        obs, info = env.reset(seed=seed + ep)
        term = False
        for t, a in enumerate(res["actions"][ep]):
            assert not term and obs["action_mask"][a] == 1, (ep, t, a)
            third = sum(env.engine.used) == 2
            obs, _, term, _, info = env.step(a)
            assert third or not term, (ep, t, "ended in the middle of a hand")
        assert term or len(res["actions"][ep]) == cut, ep
        assert res["scores"][ep] == info["score"] and res["lengths"][ep] == len(res["actions"][ep]), ep


def test_safe_random_play_replays_through_oracle(cuda):
    """What ``evaluate.py --agent random --safe-mask`` plays on the GPU: every move is legal for the oracle, and no
    oracle game ends in the middle of a hand."""
    from agents import RandomAgent
    from evaluation.evaluate import evaluate_agent

    n, seed, cut = 16, 42, 200
    res = evaluate_agent(RandomAgent(device=cuda, safe=True), num_episodes=n, seed=seed, max_moves=cut,
                         record_actions=True, safe_mask=True)
    _replay_never_ends_mid_hand(res, n, seed, cut)
    print(f"safe random play on the GPU: mean length {np.mean(res['lengths']):.1f}, mean score "
          f"{np.mean(res['scores']):.1f}")


def test_safe_mask_under_the_ppo_policy_replays_through_oracle(cuda):
    """What ``evaluate.py --agent ppo --safe-mask`` does, with an untrained network sampling: the safe words are
    AND-ed into the mask the policy samples under, so its games do not end in the middle of a hand either."""
    from agents import PPOAgent, PPOConfig
    from evaluation.evaluate import evaluate_agent

    torch.manual_seed(6)
    n, seed, cut = 16, 100, 60
    agent = PPOAgent(PPOConfig(), device=cuda, sample_seed=3)
    res = evaluate_agent(agent, num_episodes=n, deterministic=False, seed=seed, max_moves=cut, record_actions=True,
                         safe_mask=True)
    _replay_never_ends_mid_hand(res, n, seed, cut)
    print(f"untrained policy under the safe mask: mean length {np.mean(res['lengths']):.1f} of at most {cut}")
