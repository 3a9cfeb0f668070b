"""Per-action full-hand values and the hand-safe mask on the host backend (bb_plan_values of libbbvec_host.so), on
the CPU (no GPU involved), against the reference of tests/_plan_values_ref.py, which calls none of the new entry
points: all four outputs on the 92-position set at depth 1-3 under three weight sets, what ``safe`` does and does
not depend on, consistency with bb_plan_actions, argument errors, NULL outputs, the handle form, then the play
property -- random play restricted to hand-safe actions never loses in the middle of a hand -- and the CLI flag.
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
import _plan_values_ref as V

CPU = torch.device("cpu")
KEYS = ("q", "rest", "leaves", "safe")


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def ref(host):
    return R.reference()


def _host_values(ref, w, depth, idx=None, want=KEYS):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU, idx)
    return K.plan_values(board, hand, w, depth, combo=combo, want=want)


def test_reference_is_not_vacuous(ref):
    """On the reference side alone: the set has unsafe legal actions that only the search sees, positions whose
    safe set is a proper non-empty subset of the legal one, and one with legal moves and no safe one."""
    want = V.reference_values(3)
    unsafe = want["legal"] & ~want["safe"]
    hidden = unsafe & ~want["dead1"]
    n_legal, n_safe = want["legal"].sum(axis=1), want["safe"].sum(axis=1)
    proper = (n_safe > 0) & (n_safe < n_legal)
    print(f"{int(want['legal'].sum())} legal actions, {int(unsafe.sum())} unsafe, {int(hidden.sum())} of them not "
          f"dead on the spot; {int(proper.sum())} positions with a proper non-empty safe subset")
    assert unsafe.sum() >= 40 and hidden.sum() >= 22 and proper.sum() >= 6
    assert ((n_legal > 0) & (n_safe == 0)).sum() >= 1
    i = ref["names"]["dead"]
    assert n_legal[i] > 0 and n_safe[i] == 0
    assert (P.unused_slots(ref["hand"])[proper] == 3).all()  # only a whole hand hides a loss two plies away


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_host_equals_reference(ref, depth):
    from runtime import kernels as K

    want = V.reference_values(depth)
    safes = []
    for wname, w in P.WEIGHT_SETS.items():
        got = _host_values(ref, w, depth)
        V.check(got, want, wname, what=f"depth {depth}")
        safes.append(got["safe"])
    assert all(torch.equal(s, safes[0]) for s in safes[1:])  # safe does not read the weights
    i = ref["names"]["game_over"]
    assert (got["q"][i] == R.INT64_MIN).all() and (got["rest"][i] == -1).all() and (got["leaves"][i] == 0).all()
    assert (got["safe"][i] == 0).all()
    if depth == 1:
        board, hand, combo, prev = R.tensors(ref, CPU)
        aux = K.unpack_aux(K.afterstates(board, hand, combo, prev)["aux"])
        assert torch.equal(K.mask_bits_to_bool(got["safe"]), aux["legal"] & ~aux["dead"])
        assert bool(((got["rest"] == 0xFFFF) == aux["legal"]).all())
    if depth == 3:
        assert torch.equal(_host_values(ref, P.MIXED, 2, want=("safe",))["safe"], safes[0])
        assert np.array_equal(V.reference_values(2)["safe"], want["safe"])


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_consistent_with_plan_actions(ref, depth):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU)
    for wname, w in P.WEIGHT_SETS.items():
        got = _host_values(ref, w, depth)
        plan = K.plan_actions(board, hand, w, depth, combo=combo, want_plan=True, want_leaves=True)
        best = got["q"].max(dim=1).values
        assert torch.equal(best, plan["value"]), wname
        first = (got["q"] == best[:, None]).int().argmax(dim=1).int()  # the lowest action attaining the maximum
        playable = plan["leaves"] > 0
        assert torch.equal(first[playable], plan["action"][playable]), wname
        assert bool((plan["action"][~playable] == 0).all())
        a2, a3 = K.unpack_rest(got["rest"][torch.arange(ref["n"]), plan["action"].long()])
        assert torch.equal(a2[playable], plan["plan"][playable, 1]), wname
        assert torch.equal(a3[playable], plan["plan"][playable, 2]), wname
        assert torch.equal(got["leaves"].sum(dim=1).int(), plan["leaves"]), wname


def test_bad_arguments(host):
    from runtime import lib as L
    from runtime.device_env import DeviceEnvBatch

    b = np.zeros(4, np.uint64)
    h = np.zeros(4, np.uint32)
    pos = L.Positions(board=b.ctypes.data, hand=h.ctypes.data)
    w = L.greedy_weights(R.DEFAULT_WEIGHTS)
    q = np.zeros((4, 192), np.int64)
    out = L.PlanValuesOut(q=q.ctypes.data)
    ERR = -1

    def refused(rc, rule, handle=None):
        assert rc == ERR
        msg = host.bb_last_error(handle).decode()
        assert rule in msg and "bb_plan_values" in msg, msg

    for depth in (0, 4, -1):
        refused(host.bb_plan_values_pos(C.byref(pos), 4, C.byref(w), depth, C.byref(out), None), "depth")
    refused(host.bb_plan_values_pos(C.byref(pos), -3, C.byref(w), 3, C.byref(out), None), "negative")
    refused(host.bb_plan_values_pos(None, 4, C.byref(w), 3, C.byref(out), None), "positions")
    refused(host.bb_plan_values_pos(C.byref(L.Positions()), 4, C.byref(w), 3, C.byref(out), None), "positions")
    refused(host.bb_plan_values_pos(C.byref(pos), 4, None, 3, C.byref(out), None), "weights")
    refused(host.bb_plan_values_pos(C.byref(pos), 4, C.byref(w), 3, None, None), "out is NULL")
    refused(host.bb_plan_values_pos(C.byref(pos), 4, C.byref(w), 3, C.byref(L.PlanValuesOut()), None), "all four")
    q[:] = 7
    assert host.bb_plan_values_pos(C.byref(pos), 0, C.byref(w), 3, C.byref(out), None) == 0  # nothing to do
    assert (q == 7).all()
    assert host.bb_plan_values_pos(C.byref(pos), 4, C.byref(w), 3, C.byref(out), None) == 0
    assert host.bb_plan_values(None, C.byref(w), 3, C.byref(out), None) == ERR
    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    env.reset()
    for args, rule in (((None, 3, C.byref(out)), "weights"), ((C.byref(w), 0, C.byref(out)), "depth"),
                       ((C.byref(w), 4, C.byref(out)), "depth"), ((C.byref(w), 3, None), "out is NULL"),
                       ((C.byref(w), 3, C.byref(L.PlanValuesOut())), "all four")):
        refused(host.bb_plan_values(env.handle, args[0], args[1], args[2], None), rule, env.handle)
    assert host.bb_plan_values(env.handle, C.byref(w), 3, C.byref(out), None) == 0
    env.close()


def test_each_output_alone(ref):
    from runtime import kernels as K

    full = _host_values(ref, P.MIXED, 3)
    for k in KEYS:
        part = _host_values(ref, P.MIXED, 3, want=(k,))
        assert set(part) == {k} and torch.equal(part[k], full[k]), k
    board, hand, combo, _ = R.tensors(ref, CPU)
    none = K.plan_values(board, hand, P.MIXED, 3)  # combo NULL = 0
    zero = K.plan_values(board, hand, P.MIXED, 3, combo=torch.zeros_like(combo))
    assert all(torch.equal(none[k], zero[k]) for k in KEYS)
    with pytest.raises(K.L.BBNativeError):
        K.plan_values(board, hand, P.MIXED, 3, out={})
    with pytest.raises(ValueError):
        K.plan_values(board, hand, P.MIXED, 3, want=("value",))


def test_handle_form_equals_pos_form_and_leaves_the_state_alone(ref):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    n = ref["n"]
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    for depth in (1, 2, 3):
        want = _host_values(ref, P.MIXED, depth)
        out = {k: torch.full_like(v, -5) for k, v in K.plan_value_outputs(n, CPU).items()}
        assert env.plan_values(P.MIXED, depth, out=out) is out
        for k in KEYS:
            assert torch.equal(out[k], want[k]), (depth, k)
        safe = torch.full((n, 3), -5, dtype=torch.int64)
        assert env.safe_mask(safe, depth) is safe and torch.equal(safe, want["safe"])
    fresh = env.plan_values(P.MIXED)
    assert all(torch.equal(fresh[k], want[k]) for k in KEYS)
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


def test_env_surface(host):
    from environment.block_blast_env import BlockBlastEnv
    from environment.wrappers import VectorizedBlockBlastEnv

    env = BlockBlastEnv(seed=5, device="cpu")
    obs, _ = env.reset()
    pv = env.plan_values()
    legal = obs["action_mask"].astype(bool)
    assert pv["q"].shape == (192,) and np.array_equal(pv["q"] != R.INT64_MIN, legal)
    assert np.array_equal(pv["leaves"] > 0, legal) and (pv["a2"][legal] >= 0).all() and (pv["a3"][legal] >= 0).all()
    assert (pv["a2"][~legal] == -1).all() and np.array_equal(env.safe_action_mask(), pv["safe"])
    assert (pv["safe"] <= legal).all() and pv["safe"].any()
    vec = VectorizedBlockBlastEnv(3, seed=5, device="cpu")
    vec.reset()
    vv = vec.plan_values()
    assert all(np.array_equal(vv[k][0], pv[k]) for k in pv)  # env 0 of the batch has the single env's seed
    assert np.array_equal(vec.safe_action_mask(), vv["safe"]) and vv["safe"].shape == (3, 192)
    vec.close()
    env.close()


def _play(safe, seeds, moves):
    """Random play on the host backend.  Returns (terminations in the middle of a hand, games alive at the end,
    mean length, decisions whose safe set is a proper subset of the legal one, empty safe masks met right after a
    safe move that did not finish the hand)."""
    from agents import RandomAgent
    from runtime.device_env import DeviceEnvBatch

    n = len(seeds)
    env = DeviceEnvBatch(n, seeds, autoreset=False, device="cpu")
    env.reset()
    agent = RandomAgent(device="cpu", safe=safe)
    act = torch.zeros(n, dtype=torch.int32)
    legal_bits = torch.zeros((n, 3), dtype=torch.int64)
    safe_bits = torch.zeros((n, 3), dtype=torch.int64)
    alive = np.ones(n, bool)
    after_safe_open = np.zeros(n, bool)  # the last move was hand-safe and did not finish the hand
    length = np.zeros(n, np.int64)
    mid_hand = smaller = broken = 0
    for _ in range(moves):
        third = np.bitwise_count((env.state()["hand"] >> 18) & 7) == 2  # this move finishes the hand
        env.obs(mask_bits=legal_bits)
        env.safe_mask(safe_bits)
        has_safe = (safe_bits != 0).any(dim=1).numpy()
        broken += int((alive & after_safe_open & ~has_safe).sum())
        smaller += int((alive & has_safe & (safe_bits != legal_bits).any(dim=1).numpy()).sum())
        agent.act_env(env, act)
        allowed = V.safe_bool(torch.where(torch.from_numpy(has_safe)[:, None] & safe, safe_bits, legal_bits).numpy())
        assert allowed[np.arange(n), act.numpy()][alive].all()
        picked_safe = V.safe_bool(safe_bits.numpy())[np.arange(n), act.numpy()]
        env.step(act)
        term = env.terminated.numpy().astype(bool) & alive
        length += alive
        mid_hand += int((term & ~third).sum())
        alive &= ~term
        after_safe_open = picked_safe & ~third
    env.close()
    return mid_hand, int(alive.sum()), float(length.mean()), smaller, broken


def test_safe_random_play_never_loses_mid_hand(host):
    seeds, moves = list(range(42, 74)), 300
    mid_hand, alive, mean_len, smaller, broken = _play(True, seeds, moves)
    print(f"safe random play: {alive} of {len(seeds)} games alive after {moves} moves, mean length {mean_len:.1f}, "
          f"{smaller} decisions with a safe set smaller than the legal set")
    assert mid_hand == 0 and broken == 0
    assert smaller > 0  # the mask did something
    c_mid, c_alive, c_len, _, c_broken = _play(False, seeds, moves)
    print(f"control (legal mask): {c_mid} games ended in the middle of a hand, {c_alive} alive, mean length "
          f"{c_len:.1f}")
    assert c_mid >= 1 and c_broken == 0


def test_cli_safe_mask(host, tmp_path):
    from runtime.device_env import DeviceEnvBatch

    pkg = os.path.dirname(os.path.abspath(sys.modules["runtime"].__file__))
    base = [sys.executable, os.path.join(os.path.dirname(pkg), "evaluate.py"), "--agent", "random", "--device", "cpu",
            "--episodes", "8", "--max-moves", "200"]
    res = {}
    for name, extra in (("safe", ["--safe-mask"]), ("plain", [])):
        out = tmp_path / f"{name}.json"
        run = subprocess.run(base + extra + ["--output", str(out)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        assert "Baseline agent: random" in run.stdout and "EVALUATION RESULTS" in run.stdout
        assert ("hand-safe" in run.stdout) == (name == "safe")
        res[name] = json.load(open(out))
        assert res[name]["num_episodes"] == 8 and max(res[name]["lengths"]) <= 200
    print(f"mean length: {np.mean(res['safe']['lengths']):.1f} with --safe-mask, "
          f"{np.mean(res['plain']['lengths']):.1f} without")
    # without the flag: the games of the legal-mask Philox policy on seeds 42..49, played here move by move
    n = 8
    env = DeviceEnvBatch(n, [42 + e for e in range(n)], autoreset=False, device="cpu")
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64)
    act = torch.zeros(n, dtype=torch.int32)
    alive = np.ones(n, bool)
    length = np.zeros(n, np.int64)
    for step in range(200):
        env.obs(mask_bits=mb)
        env.random_actions(mb, act, step=step)
        env.step(act)
        length += alive
        alive &= ~env.terminated.numpy().astype(bool)
    scores = env.state()["score"]
    env.close()
    assert res["plain"]["lengths"] == length.tolist() and res["plain"]["scores"] == scores.tolist()
