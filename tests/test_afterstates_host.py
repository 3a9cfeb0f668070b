"""One-ply lookahead on the host backend (bb_afterstates / bb_greedy_actions of libbbvec_host.so, csrc/bb_host.cpp)
against the unmodified oracle, on the CPU (no GPU involved).

The expectation and the position set are tests/_afterstates_ref.py's: for every position ``copy.deepcopy`` of the
``oracle.bb_game.Env`` that holds it and ``step(a)`` for each of the 192 actions (a refill move with the chance
part removed), played positions from 16 games stepped in lockstep plus crafted ones.  All four outputs are
compared for every action, legal or not; the fp64 reward with ``==``.  Then the fused greedy choice against a
numpy arg-max over the oracle's features, the argument checks, the handle form against the stateless form, the
baseline agents through ``evaluate_agent`` with the greedy games replayed through the oracle, and the CLI.
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
from oracle import bb_game as O

CPU = torch.device("cpu")
WEIGHT_SETS = {
    "default": R.DEFAULT_WEIGHTS,
    "zero": {},  # every legal action ties: the lowest one must be chosen
    "mixed": {"lines": -7, "score": 3, "holes": -1, "filled": 1, "centre": 5, "mobility": -2, "dead": 50,
              "refill": 11},
}


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def ref(host):
    return R.reference()


def test_afterstates_match_oracle_for_every_action(ref):
    from runtime import kernels as K

    out = K.afterstates(*R.tensors(ref, CPU))
    R.check_dense(ref, out, what="host _pos")
    legal = ref["legal"]
    n_legal = int(legal.sum())
    classes = {
        "illegal": int((~legal).sum()),
        "refill": int((legal & (ref["refill"] == 1)).sum()),
        "dead": int((legal & (ref["dead"] == 1)).sum()),
        "lines>=2": int((legal & (ref["lines"] >= 2)).sum()),
        "capped combo": int((legal & ref["capped"]).sum()),
    }
    # the hole penalty and the centre bonus, each on and off, among the compared legal actions
    prev_h = (ref["prev"] & 0xFF).astype(np.int64)[:, None]
    prev_c = (ref["prev"] >> 8).astype(np.int64)[:, None]
    classes["hole penalty on"] = int((legal & (ref["holes"] > prev_h)).sum())
    classes["hole penalty off"] = int((legal & (ref["holes"] <= prev_h)).sum())
    classes["centre bonus on"] = int((legal & (ref["centre"] <= prev_c)).sum())
    classes["centre bonus off"] = int((legal & (ref["centre"] > prev_c)).sum())
    skipped = int(ref["chance_end"].sum())
    print(f"{ref['n']} positions, {n_legal} legal actions compared; classes {classes}; "
          f"{skipped} refill rewards left out (the real step's new hand ends the game)")
    for name, count in classes.items():
        assert count > 0, f"the position set holds no {name} action"
    assert skipped * 100 <= n_legal, (skipped, n_legal)
    # the crafted positions are what they were built to be
    names = ref["names"]
    i = names["row_and_column"]
    assert ref["lines"][i, 0] == 2 and ref["exp_board"][i, 0] == 0
    i = names["combo9"]  # 1 + (2*8*10) * min(2,4) * min(10+1, 8)
    assert ref["capped"][i, 0] and ref["exp_score"][i, 0] == 1 + 160 * 2 * 8
    i = names["dead"]
    assert legal[i].sum() == 16 and (ref["dead"][i][legal[i]] == 1).all()
    assert not legal[names["game_over"]].any()


@pytest.mark.parametrize("wname", list(WEIGHT_SETS))
def test_greedy_actions_match_numpy_argmax(ref, wname):
    from runtime import kernels as K

    w = WEIGHT_SETS[wname]
    board, hand, combo, _ = R.tensors(ref, CPU)
    action, value = K.greedy_actions(board, hand, w, combo=combo)
    want_a, want_v = R.expected_greedy(ref, w)
    assert np.array_equal(action.numpy(), want_a), wname
    assert np.array_equal(value.numpy(), want_v), wname
    if wname == "zero":  # the tie-break decides every choice
        first = np.where(ref["legal"].any(1), ref["legal"].argmax(1), 0)
        assert np.array_equal(action.numpy(), first)
    i = ref["names"]["game_over"]  # no legal action: 0 and INT64_MIN
    assert action[i] == 0 and value[i] == R.INT64_MIN
    a2, v2 = K.greedy_actions(board, hand, w, combo=combo, want_value=False)
    assert v2 is None and np.array_equal(a2.numpy(), want_a)


def test_optional_outputs_and_optional_columns(ref):
    from runtime import kernels as K

    board, hand, combo, prev = R.tensors(ref, CPU)
    full = K.afterstates(board, hand, combo, prev)
    for k in ("board", "reward", "score_gained", "aux"):
        one = K.afterstates(board, hand, combo, prev, out=K.afterstate_outputs(ref["n"], CPU, want=(k,)))
        assert list(one) == [k] and torch.equal(one[k], full[k]), k
    # combo / prev NULL mean 0
    zero = K.afterstates(board, hand, torch.zeros_like(combo), torch.zeros_like(prev))
    none = K.afterstates(board, hand)
    for k in full:
        assert torch.equal(zero[k], none[k]), k


def test_bad_arguments(host):
    from runtime import lib as L

    b = np.zeros(4, np.uint64)
    h = np.zeros(4, np.uint32)
    pos = L.Positions(board=b.ctypes.data, hand=h.ctypes.data)
    out = L.AfterstateOut()
    cfg = L.reward_cfg(R.O.DEFAULT_REWARDS)
    w = L.greedy_weights(R.DEFAULT_WEIGHTS)
    act = np.zeros(4, np.int32)
    ap = act.ctypes.data_as(C.c_void_p)
    BB_ERR_ARG = -1
    for n in (0, -3):
        assert host.bb_afterstates_pos(C.byref(pos), n, C.byref(cfg), C.byref(out), None) == BB_ERR_ARG
        assert host.bb_greedy_actions_pos(C.byref(pos), n, C.byref(w), ap, None, None) == BB_ERR_ARG
    assert host.bb_afterstates_pos(None, 4, C.byref(cfg), C.byref(out), None) == BB_ERR_ARG
    assert host.bb_greedy_actions_pos(None, 4, C.byref(w), ap, None, None) == BB_ERR_ARG
    assert host.bb_afterstates_pos(C.byref(L.Positions()), 4, C.byref(cfg), C.byref(out), None) == BB_ERR_ARG
    assert host.bb_afterstates_pos(C.byref(pos), 4, None, C.byref(out), None) == BB_ERR_ARG
    assert host.bb_afterstates_pos(C.byref(pos), 4, C.byref(cfg), None, None) == BB_ERR_ARG
    assert host.bb_greedy_actions_pos(C.byref(pos), 4, None, ap, None, None) == BB_ERR_ARG
    assert host.bb_greedy_actions_pos(C.byref(pos), 4, C.byref(w), None, None, None) == BB_ERR_ARG
    assert b"bb_greedy_actions_pos" in host.bb_last_error(None)
    assert host.bb_afterstates(None, C.byref(out), None) == BB_ERR_ARG
    assert host.bb_greedy_actions(None, C.byref(w), ap, None, None) == BB_ERR_ARG
    with pytest.raises(ValueError):
        L.greedy_weights({"speed": 1})


def test_handle_form_equals_pos_form_and_leaves_the_state_alone(ref):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    n = ref["n"]
    rw = {"line_clear_base": 2.5, "block_placed": 0.03, "game_over_penalty": -3.0, "hole_penalty": -0.25,
          "center_bonus": 0.7, "combo_multiplier_bonus": 1.25, "survival_bonus": 0.0625}
    env = DeviceEnvBatch(n, list(range(n)), reward_config=rw, autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    got = env.afterstates()
    act = torch.zeros(n, dtype=torch.int32)
    val = torch.zeros(n, dtype=torch.int64)
    env.greedy_actions(act, WEIGHT_SETS["mixed"], value=val)
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    board, hand, combo, prev = R.tensors(ref, CPU)
    want = K.afterstates(board, hand, combo, prev, reward_config=rw)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(want["reward"], K.afterstates(board, hand, combo, prev)["reward"])  # the handle's config
    a2, v2 = K.greedy_actions(board, hand, WEIGHT_SETS["mixed"], combo=combo)
    assert torch.equal(act, a2) and torch.equal(val, v2)
    env.close()


def test_gym_surface_afterstates_agree_with_step(host):
    """BlockBlastEnv.afterstates() / VectorizedBlockBlastEnv.afterstates() on the host backend: the unpacked
    arrays, and the reward / termination of the move then played (a non-refill move: no chance part)."""
    from environment.block_blast_env import BlockBlastEnv
    from environment.wrappers import VectorizedBlockBlastEnv

    env = BlockBlastEnv(seed=5, device="cpu")
    obs, _ = env.reset()
    af = env.afterstates()
    assert set(af) == {"board", "reward", "score_gained", "legal", "dead", "refill", "lines", "holes", "centre",
                       "mobility"}
    assert all(v.shape == (192,) for v in af.values())
    assert np.array_equal(af["legal"], obs["action_mask"].astype(bool))
    a = int(np.nonzero(af["legal"])[0][7])
    _, reward, term, _, info = env.step(a)
    assert reward == af["reward"][a] and term == bool(af["dead"][a]) and not af["refill"][a]
    assert info["last_move"]["score_gained"] == af["score_gained"][a] and info["holes"] == af["holes"][a]
    vec = VectorizedBlockBlastEnv(3, seed=5, device="cpu")
    vobs, _ = vec.reset()
    vaf = vec.afterstates()
    assert vaf["board"].shape == (3, 192) and vaf["board"].dtype == np.uint64
    assert np.array_equal(vaf["legal"], vobs["action_mask"].astype(bool))
    assert np.array_equal(vaf["reward"][0], af["reward"])  # env 0 is seeded 5 too
    vec.close()


def _replay_score(actions, seed, cut):
    """The oracle's game for one recorded episode: every action legal, the game ends exactly at the recorded
    length unless the evaluation cut it off at ``cut`` moves; returns the oracle's score."""
    env = O.Env(seed=seed)
    obs, info = env.reset(seed=seed)
    term = False
    for t, a in enumerate(actions):
        assert not term and obs["action_mask"][a] == 1, (seed, t, a)
        obs, _, term, _, info = env.step(a)
    assert term or len(actions) == cut, seed
    return info["score"]


def test_greedy_agent_beats_random_play_and_replays_through_the_oracle(host, tmp_path):
    from agents import GreedyAgent, RandomAgent
    from evaluation.evaluate import evaluate_agent

    n, seed, cut = 32, 42, 150
    agent = GreedyAgent(device="cpu")
    assert agent.weights == R.DEFAULT_WEIGHTS and agent.update() == {}
    path = str(tmp_path / "greedy.json")
    agent.save(path)
    assert json.load(open(path))["weights"] == R.DEFAULT_WEIGHTS
    other = GreedyAgent({"lines": 1}, device="cpu")
    other.load(path)
    assert other.weights == agent.weights
    greedy = evaluate_agent(agent, num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    rand = evaluate_agent(RandomAgent(device="cpu"), num_episodes=n, seed=seed, max_moves=cut, record_actions=True)
    for res in (greedy, rand):
        for ep in range(n):
            assert res["lengths"][ep] == len(res["actions"][ep]) <= cut
            assert res["scores"][ep] == _replay_score(res["actions"][ep], seed + ep, cut), ep
    print(f"greedy mean score {greedy['mean_score']:.1f} (length {greedy['mean_length']:.1f}), "
          f"random {rand['mean_score']:.1f} (length {rand['mean_length']:.1f})")
    assert greedy["mean_score"] > rand["mean_score"]
    # the single-observation path picks what the fused path picks
    from environment.block_blast_env import BlockBlastEnv

    env = BlockBlastEnv(seed=seed, device="cpu")
    obs, _ = env.reset()
    for a in greedy["actions"][0][:6]:
        assert agent.select_action(obs)[0] == a
        obs = env.step(a)[0]


def test_cli_baseline_writes_the_usual_keys(host, tmp_path):
    pkg = os.path.dirname(os.path.abspath(sys.modules["runtime"].__file__))
    out = tmp_path / "greedy.json"
    cmd = [sys.executable, os.path.join(os.path.dirname(pkg), "evaluate.py"), "--agent", "greedy", "--episodes", "4",
           "--max-moves", "50", "--device", "cpu", "--output", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "EVALUATION RESULTS" in run.stdout
    res = json.load(open(out))
    assert set(res) == {"num_episodes", "mean_score", "std_score", "min_score", "max_score", "median_score",
                        "mean_length", "std_length", "mean_lines_cleared", "mean_max_combo", "scores", "lengths"}
    assert res["num_episodes"] == 4 and len(res["scores"]) == 4 and max(res["lengths"]) <= 50
    # --agent ppo still asks for its checkpoint
    run = subprocess.run(cmd[:2] + ["--episodes", "1"], capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "--checkpoint" in run.stderr
