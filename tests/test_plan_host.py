"""Full-hand lookahead on the host backend (bb_plan_actions of libbbvec_host.so, the DFS of csrc/bb_host.cpp), on
the CPU (no GPU involved), against two references that call none of the new entry points (tests/_plan_ref.py):

* the chained one-ply reference (``K.afterstates`` level by level + numpy) on the 92-position set of
  tests/_afterstates_ref.py, depth 1-3, three weight sets, all four outputs equal;
* the oracle brute force (``copy.deepcopy(env).step(a)`` recursion) on the small-tree positions at depth 3.

Then depth 1 against the greedy call, "the plan stays the plan" through bb_step, argument errors, NULL optional
outputs, the handle form, the agent and the CLI.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _plan_ref as P

CPU = torch.device("cpu")
SMALL_TREE = 3200  # leaves at depth 3 the oracle brute force is run up to (the crafted "prev_switch" has 3,191)


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def ref(host):
    return R.reference()


def _host_plan(ref, w, depth, idx=None):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU, idx)
    return K.plan_actions(board, hand, w, depth, combo=combo, want_plan=True, want_leaves=True)


def test_position_set_is_not_vacuous(ref):
    want = P.reference_plans(3)
    slots = P.unused_slots(ref["hand"])
    playable = want["default"]["leaves"] > 0
    for k in (1, 2, 3):
        assert (playable & (slots == k)).any(), f"no playable position with {k} unused slots"
    late_clear = False
    for i in np.nonzero(want["default"]["plan"][:, 1] >= 0)[0]:
        lines, _ = P.plan_lines(ref["board"][i], ref["hand"][i], ref["combo"][i], want["default"]["plan"][i])
        late_clear |= any(x > 0 for x in lines[1:])
    assert late_clear, "no best plan clears a line at ply 2 or 3"
    assert want["_stats"]["dead_before_depth"].any(), "no maximal sequence ends dead before the depth"
    i = ref["names"]["game_over"]
    assert want["default"]["leaves"][i] == 0 and want["default"]["value"][i] == R.INT64_MIN
    print(f"{ref['n']} positions; leaves at depth 3: mean {want['default']['leaves'].mean():.0f}, "
          f"max {want['default']['leaves'].max()}")


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("wname", list(P.WEIGHT_SETS))
def test_host_equals_chained_reference(ref, depth, wname):
    want = P.reference_plans(depth)[wname]
    got = _host_plan(ref, P.WEIGHT_SETS[wname], depth)
    for k in ("leaves", "value", "plan", "action"):
        g = got[k].numpy()
        bad = np.nonzero((g != want[k]).reshape(ref["n"], -1).any(axis=1))[0]
        assert bad.size == 0, (k, depth, wname, bad[:4].tolist(), g[bad[:4]].tolist(), want[k][bad[:4]].tolist())
    i = ref["names"]["game_over"]
    assert got["action"][i] == 0 and got["value"][i] == R.INT64_MIN and got["leaves"][i] == 0
    assert got["plan"][i].tolist() == [-1, -1, -1]
    if wname == "zero":  # every value is 0: the lexicographically lowest maximal sequence
        assert (got["value"].numpy()[want["leaves"] > 0] == 0).all()


def test_host_equals_oracle_brute_force_on_small_trees(ref):
    leaves = P.reference_plans(3)["default"]["leaves"]
    crafted = sorted(ref["names"].values())
    slots = P.unused_slots(ref["hand"])
    small = [int(i) for i in np.argsort(leaves, kind="stable") if i not in crafted and 0 < leaves[i] <= SMALL_TREE]
    played = [i for k in (1, 2, 3) for i in [j for j in small if slots[j] == k][:3]]  # the smallest of each kind
    idx = [i for i in crafted if leaves[i] <= SMALL_TREE] + played
    print(f"oracle brute force on {len(idx)} positions, leaves {leaves[idx].tolist()}, unused slots "
          f"{slots[idx].tolist()}")
    assert len(idx) >= 10 and {1, 2, 3} <= set(slots[idx].tolist()), (idx, leaves[idx].tolist())
    deep = 0
    for wname in ("default", "mixed"):
        got = _host_plan(ref, P.WEIGHT_SETS[wname], 3, np.array(idx))
        for j, i in enumerate(idx):
            value, plan, count = P.oracle_search(ref["envs"][i], 3, P.WEIGHT_SETS[wname])
            assert got["leaves"][j] == count, (wname, i)
            assert got["value"][j] == value and got["plan"][j].tolist() == plan, (wname, i, plan)
            deep += plan[1] >= 0
    assert deep > 0


def test_depth_one_is_greedy(ref):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU)
    one_slot = torch.from_numpy(P.unused_slots(ref["hand"]) == 1)
    assert one_slot.any()
    for w in P.WEIGHT_SETS.values():
        ga, gv = K.greedy_actions(board, hand, w, combo=combo)
        got = _host_plan(ref, w, 1)
        assert torch.equal(got["action"], ga) and torch.equal(got["value"], gv)
        assert (got["plan"][:, 1:] == -1).all()
        deep = _host_plan(ref, w, 3)  # one unused slot: every first move is a refill move
        assert torch.equal(deep["action"][one_slot], ga[one_slot]) and torch.equal(deep["value"][one_slot], gv[one_slot])


def test_the_plan_stays_the_plan(ref):
    """After a_1 is played through bb_step, the search one ply shallower on the live state returns (a_2[, a_3]),
    and its value is the old one minus the move terms of a_1."""
    from runtime.device_env import DeviceEnvBatch

    w = P.MIXED
    first = _host_plan(ref, w, 3)
    idx = np.nonzero(first["plan"][:, 1].numpy() >= 0)[0]
    assert len(idx) >= 8 and (first["plan"][idx, 2].numpy() >= 0).any()
    n = len(idx)
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    env.step(first["action"][idx].contiguous(), want_info=True)
    assert not env.terminated.bool().any()  # a_2 exists: a_1 neither refilled nor ended the game
    act = torch.zeros(n, dtype=torch.int32)
    val = torch.zeros(n, dtype=torch.int64)
    plan = torch.zeros((n, 3), dtype=torch.int32)
    env.plan_actions(act, w, depth=2, value=val, plan=plan)
    env.close()
    for j, i in enumerate(idx):
        lines, gained = P.plan_lines(ref["board"][i], ref["hand"][i], ref["combo"][i], first["plan"][i].tolist())
        assert plan[j].tolist() == first["plan"][i, 1:].tolist() + [-1], i
        assert int(val[j]) == int(first["value"][i]) - (w["lines"] * lines[0] + w["score"] * gained[0]), i


def test_bad_arguments(host):
    from runtime import lib as L

    b = np.zeros(4, np.uint64)
    h = np.zeros(4, np.uint32)
    pos = L.Positions(board=b.ctypes.data, hand=h.ctypes.data)
    w = L.greedy_weights(R.DEFAULT_WEIGHTS)
    act = np.zeros(4, np.int32)
    out = L.PlanOut(action=act.ctypes.data)
    ERR = -1
    for depth in (0, 4, -1):
        assert host.bb_plan_actions_pos(C.byref(pos), 4, C.byref(w), depth, C.byref(out), None) == ERR
    assert b"bb_plan_actions_pos" in host.bb_last_error(None)
    for n in (0, -3):
        assert host.bb_plan_actions_pos(C.byref(pos), n, C.byref(w), 3, C.byref(out), None) == ERR
    assert host.bb_plan_actions_pos(None, 4, C.byref(w), 3, C.byref(out), None) == ERR
    assert host.bb_plan_actions_pos(C.byref(L.Positions()), 4, C.byref(w), 3, C.byref(out), None) == ERR
    assert host.bb_plan_actions_pos(C.byref(pos), 4, None, 3, C.byref(out), None) == ERR
    assert host.bb_plan_actions_pos(C.byref(pos), 4, C.byref(w), 3, None, None) == ERR
    assert host.bb_plan_actions_pos(C.byref(pos), 4, C.byref(w), 3, C.byref(L.PlanOut()), None) == ERR
    assert host.bb_plan_actions_pos(C.byref(pos), 4, C.byref(w), 3, C.byref(out), None) == 0
    assert host.bb_plan_actions(None, C.byref(w), 3, C.byref(out), None) == ERR
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    env.reset()
    for args in ((None, 3, C.byref(out)), (C.byref(w), 0, C.byref(out)), (C.byref(w), 4, C.byref(out)),
                 (C.byref(w), 3, None), (C.byref(w), 3, C.byref(L.PlanOut()))):
        assert host.bb_plan_actions(env.handle, args[0], args[1], args[2], None) == ERR
        assert b"bb_plan_actions" in host.bb_last_error(env.handle)
    assert host.bb_plan_actions(env.handle, C.byref(w), 3, C.byref(out), None) == 0
    env.close()


def test_optional_outputs_null_one_at_a_time(ref):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU)
    full = K.plan_actions(board, hand, P.MIXED, 3, combo=combo, want_plan=True, want_leaves=True)
    wants = {"value": "want_value", "plan": "want_plan", "leaves": "want_leaves"}
    for skip in wants:
        part = K.plan_actions(board, hand, P.MIXED, 3, combo=combo, **{v: k != skip for k, v in wants.items()})
        assert set(part) == set(full) - {skip}
        for k in part:
            assert torch.equal(part[k], full[k]), (skip, k)
    only = K.plan_actions(board, hand, P.MIXED, 3, combo=combo, want_value=False)
    assert set(only) == {"action"} and torch.equal(only["action"], full["action"])
    none = K.plan_actions(board, hand, P.MIXED, 3, want_plan=True)  # combo NULL = 0
    zero = K.plan_actions(board, hand, P.MIXED, 3, combo=torch.zeros_like(combo), want_plan=True)
    assert torch.equal(none["plan"], zero["plan"]) and torch.equal(none["value"], zero["value"])


def test_handle_form_equals_pos_form_and_leaves_the_state_alone(ref):
    from runtime.device_env import DeviceEnvBatch

    n = ref["n"]
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    for depth in (1, 2, 3):
        want = _host_plan(ref, P.MIXED, depth)
        act = torch.full((n,), -5, dtype=torch.int32)
        val = torch.zeros(n, dtype=torch.int64)
        plan = torch.zeros((n, 3), dtype=torch.int32)
        leaves = torch.zeros(n, dtype=torch.int32)
        assert env.plan_actions(act, P.MIXED, depth, value=val, plan=plan, leaves=leaves) is act
        for k, t in (("action", act), ("value", val), ("plan", plan), ("leaves", leaves)):
            assert torch.equal(t, want[k]), (depth, k)
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


def test_plan_agent_plays_legal_games_and_depth_one_is_greedy(host, tmp_path):
    from agents import DEFAULT_WEIGHTS, GreedyAgent, HandPlanAgent
    from environment.block_blast_env import BlockBlastEnv
    from evaluation.evaluate import evaluate_agent
    from test_afterstates_host import _replay_score

    n, seed, cut = 6, 42, 30
    agent = HandPlanAgent(device="cpu")
    assert agent.weights == DEFAULT_WEIGHTS and agent.depth == 3 and agent.update() == {}
    path = str(tmp_path / "plan.json")
    HandPlanAgent({"lines": 7}, depth=2, device="cpu").save(path)
    saved = json.load(open(path))
    assert saved["agent"] == "plan" and saved["depth"] == 2 and saved["weights"]["lines"] == 7
    other = HandPlanAgent(device="cpu")
    other.load(path)
    assert other.depth == 2 and other.weights["lines"] == 7
    with pytest.raises(ValueError):
        HandPlanAgent(depth=4, device="cpu")
    res = evaluate_agent(agent, num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    for ep in range(n):
        assert res["lengths"][ep] == len(res["actions"][ep]) <= cut
        assert res["scores"][ep] == _replay_score(res["actions"][ep], seed + ep, cut), ep
    one = evaluate_agent(HandPlanAgent(depth=1, device="cpu"), num_episodes=n, seed=seed, max_moves=cut,
                         record_actions=True)
    greedy = evaluate_agent(GreedyAgent(device="cpu"), num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    assert one["actions"] == greedy["actions"]
    # the single-observation path picks what the fused path picks (the default weights do not read the combo)
    env = BlockBlastEnv(seed=seed, device="cpu")
    obs, _ = env.reset()
    for a in res["actions"][0][:4]:
        got, extra = agent.select_action(obs)
        assert got == a and extra["plan"][0] == a
        obs = env.step(a)[0]


def test_cli_plan_agent(host, tmp_path):
    pkg = os.path.dirname(os.path.abspath(sys.modules["runtime"].__file__))
    out = tmp_path / "plan.json"
    cmd = [sys.executable, os.path.join(os.path.dirname(pkg), "evaluate.py"), "--agent", "plan", "--depth", "2",
           "--episodes", "3", "--max-moves", "20", "--device", "cpu", "--output", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "Baseline agent: plan" in run.stdout and "EVALUATION RESULTS" in run.stdout
    res = json.load(open(out))
    assert res["num_episodes"] == 3 and max(res["lengths"]) <= 20
    run = subprocess.run(cmd[:4] + ["--depth", "4"], capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "--depth" in run.stderr
