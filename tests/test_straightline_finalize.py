"""The select-only reward (bb_rules.h move_reward), the branch-free masks_of and the rollout kernel's
straight-line finalize (csrc/bb_env.hip), bit for bit against the oracles.

These rewrites compute every term for every lane and commit by select, so the places where a select could
differ from the branch it replaced are pinned here:

* the shaped reward in fp64 under reward configs that make a wrongly committed term visible (every
  coefficient negative; zero and minus-zero coefficients beside non-zero hole and game-over terms), on the
  host backend, which shares move_reward with the kernels;
* the 192-bit masks with 0, 1 and 2 used slots and with game-over hands (masks_of reads the rows of used
  slots too and selects them away), in a second workgroup with a full and a partly live env wave;
* the invalid action, which is a select in the rollout kernel: reward -10, nothing else changes.

The GPU shapes are the smallest that reach those paths: 300 envs are two workgroups (256 + 44: one full env
wave and one of 44 lanes in the second), three launches of 12 steps carry hand, stream and mask across launch
boundaries at every hand phase, and boards filled to 0.6 and 0.9 end games within the 36 steps.
"""
import numpy as np
import pytest
import torch

from _crowded import crowded_setup
from oracle import bb_game as O
from oracle import c_oracle as CO

SEED = 0xB10C

# every coefficient negative: a term committed without its condition lowers the reward visibly
CONFIG_A = {"line_clear_base": -1.5, "block_placed": -0.03, "game_over_penalty": -3.0, "hole_penalty": -0.25,
            "center_bonus": -0.7, "combo_multiplier_bonus": -1.25, "survival_bonus": -0.0625}
# zero and minus-zero coefficients: the sums of the first steps are signed zeros, beside non-zero hole and
# game-over terms
CONFIG_B = {"block_placed": -0.0, "survival_bonus": 0.0, "center_bonus": -0.0, "hole_penalty": -0.25,
            "game_over_penalty": -3.0}
CONFIGS = {"default": None, "A": CONFIG_A, "B": CONFIG_B}


# --------------------------------------------------------------------------
# CPU: the host backend's fp64 reward against the Python oracle
# --------------------------------------------------------------------------
def _pick_actions(envs, rng, p_invalid=0.12):
    """A legal action per env, or with p_invalid one of the four invalid kinds: -1, 192, an illegal anchor on
    a filled cell for an unused slot, any anchor of a used slot (-1 or 192 where the position offers none)."""
    acts = np.zeros(len(envs), np.int32)
    invalid = np.zeros(len(envs), bool)
    for i, e in enumerate(envs):
        g = e.engine
        legal = np.nonzero(e.obs()["action_mask"])[0]
        acts[i] = rng.choice(legal)
        if rng.random() >= p_invalid:
            continue
        kind = int(rng.integers(4))
        mask = e.obs()["action_mask"]
        used = [s for s in range(3) if g.used[s]]
        occupied = [64 * s + r * 8 + c for s in range(3) if not g.used[s] for r in range(8) for c in range(8)
                    if g.grid[r][c] and not mask[64 * s + r * 8 + c]]
        if kind == 2 and occupied:
            acts[i] = int(rng.choice(occupied))
        elif kind == 3 and used:
            acts[i] = 64 * int(rng.choice(used)) + int(rng.integers(64))
        else:
            acts[i] = -1 if kind % 2 == 0 else 192
        invalid[i] = True
    return acts, invalid


@pytest.mark.parametrize("name", list(CONFIGS))
def test_host_reward_bits_match_python_oracle(name):
    from runtime.build import build_host_lib
    from runtime.device_env import DeviceEnvBatch

    build_host_lib(verbose=False)
    n, steps, rw = 64, 60, CONFIGS[name]
    env = DeviceEnvBatch(n, seeds=[42 + i for i in range(n)], device="cpu", reward_config=rw)
    env.reset()
    refs = [O.Env(reward_config=rw, seed=42 + i) for i in range(n)]
    for e in refs:
        e.reset()
    rng = np.random.default_rng(11)
    n_invalid = n_lines = n_over = 0
    for t in range(steps):
        acts, invalid = _pick_actions(refs, rng)
        env.step(torch.from_numpy(acts), want_f64=True, want_lines=True)
        want = np.zeros(n, np.float64)
        term = np.zeros(n, bool)
        for i, e in enumerate(refs):
            _, want[i], term[i], _, info = e.step(int(acts[i]))
            assert info["invalid_action"] == bool(invalid[i]), (t, i)
            if term[i]:
                e.reset()  # the batch auto-resets (wrappers.py:97-102)
        got = env.reward_f64.numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, t)
        assert np.array_equal(env.terminated.numpy().astype(bool), term), (name, t)
        assert (got[invalid] == -10.0).all() and not term[invalid].any(), (name, t)
        n_invalid += int(invalid.sum())
        n_lines += int((env.lines.numpy() > 0).sum())
        n_over += int(term.sum())
    assert n_invalid > 100 and n_lines > 50  # both arms of the valid and the line selects ran
    env.close()


# --------------------------------------------------------------------------
# GPU: crowded starts, rollout against chained steps and the C oracle
# --------------------------------------------------------------------------
N, T, LAUNCHES = 300, 12, 3
_START = {}
_REF = {}


def _start():
    """300 crowded boards and hands (tests/_crowded.py), 150 at fill 0.6 and 150 at 0.9, and the first actions.
    Both sides reset first and then take board and hand, so env i's stream is default_rng(5000 + i) after the
    reset's draws, and everything else is a fresh episode's."""
    if not _START:
        lo, a_lo, _ = crowded_setup(0.6, N // 2)
        hi, a_hi, _ = crowded_setup(0.9, N - N // 2)
        _START["state"] = {k: np.concatenate([lo[k], hi[k]]) for k in ("board", "hand")}
        _START["acts"] = np.concatenate([a_lo, a_hi])
    return _START["state"], _START["acts"]


def _seeds(n=N):
    return np.arange(5000, 5000 + n, dtype=np.uint64)


def _oracle_env(name, n=N):
    state, _ = _start()
    c = CO.CVecEnv(_seeds(n), reward_config=CONFIGS[name])
    c.reset()
    c.set_board_hand(board=state["board"][:n], hand=state["hand"][:n])
    return c


def _device_env(device, name, n=N):
    from runtime.device_env import DeviceEnvBatch

    state, _ = _start()
    env = DeviceEnvBatch(n, seeds=[int(s) for s in _seeds(n)], device=device, reward_config=CONFIGS[name])
    env.reset()
    has32 = env.state()["hand"] & np.uint32(1 << 22)  # the stream's buffered half survives the new hand
    env.set_state(board=state["board"][:n], hand=state["hand"][:n] | has32)
    return env


def _oracle(name):
    """The C oracle's three launches from the crowded starts, computed once per reward config."""
    if name not in _REF:
        _, acts = _start()
        c = _oracle_env(name)
        outs, a = [], acts
        for k in range(LAUNCHES):
            outs.append(c.rollout(T, a, policy_seed=SEED, policy_step0=k * T))
            a = outs[-1]["next_action"]
        ref = {key: np.concatenate([o[key] for o in outs]) for key in ("reward", "terminated", "lines", "actions",
                                                                        "mask")}
        ref["next_action"] = a
        _REF[name] = (ref, c.state())
        c.close()
    return _REF[name]


def _gpu_env(cuda, name):
    return _device_env(cuda, name), torch.tensor(_start()[1], dtype=torch.int32, device=cuda)  # a copy


def _gpu_rollout(cuda, name):
    env, a = _gpu_env(cuda, name)
    nxt = torch.zeros_like(a)
    steps = T * LAUNCHES
    out = {"reward": torch.zeros((steps, N), dtype=torch.float32, device=cuda),
           "terminated": torch.zeros((steps, N), dtype=torch.uint8, device=cuda),
           "lines": torch.zeros((steps, N), dtype=torch.uint8, device=cuda),
           "actions": torch.zeros((steps, N), dtype=torch.int32, device=cuda),
           "mask": torch.zeros((steps, N, 3), dtype=torch.int64, device=cuda)}
    for k in range(LAUNCHES):
        lo, hi = k * T, (k + 1) * T
        env.rollout(T, a, out["reward"][lo:hi], out["terminated"][lo:hi], lines=out["lines"][lo:hi],
                    actions_out=out["actions"][lo:hi], mask_out=out["mask"][lo:hi], next_action=nxt,
                    policy_seed=SEED, policy_step0=lo)
        a, nxt = nxt, a
        env.sync()  # raises if a wave left through an iteration cap
    return _finish(env, out, a, cuda)


def _gpu_chained(cuda, name):
    env, a = _gpu_env(cuda, name)
    nxt = torch.zeros_like(a)
    mb = torch.zeros((N, 3), dtype=torch.int64, device=cuda)
    rew, term, lines, acts, masks = [], [], [], [], []
    for t in range(T * LAUNCHES):
        acts.append(a.clone())
        env.step(a, next_action=nxt, want_lines=True, policy_seed=SEED, policy_step=t + 1, mask_out=mb)
        rew.append(env.reward.clone())
        term.append(env.terminated.clone())
        lines.append(env.lines.clone())
        masks.append(mb.clone())
        a, nxt = nxt, a
    out = {"reward": torch.stack(rew), "terminated": torch.stack(term), "lines": torch.stack(lines),
           "actions": torch.stack(acts), "mask": torch.stack(masks)}
    return _finish(env, out, a, cuda)


def _finish(env, out, a, cuda):
    env.sync()
    mb = torch.zeros((N, 3), dtype=torch.int64, device=cuda)
    env.obs(mask_bits=mb)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["mask"] = out["mask"].view(np.uint64)
    out["next_action"] = a.cpu().numpy()
    st = env.state()
    st["mask"] = mb.cpu().numpy().view(np.uint64)
    env.close()
    return out, st


def _assert_same(ref, got, what):
    (ro, rs), (go, gs) = ref, got
    for k in ("reward", "terminated", "lines", "actions", "mask", "next_action"):
        a, b = (ro[k].view(np.uint32), go[k].view(np.uint32)) if k == "reward" else (ro[k], go[k])
        assert np.array_equal(a, b), f"{what}: {k}"
    for k in ("board", "hand", "score", "combo", "max_combo", "moves", "lines", "blocks", "prev_holes",
              "prev_center", "mask"):
        assert np.array_equal(rs[k], gs[k]), f"{what}: state {k}"
    assert np.array_equal(rs["rng"][:, :2], gs["rng"][:, :2]), f"{what}: pcg state"
    has = ((rs["hand"] >> np.uint32(22)) & np.uint32(1)).astype(bool)  # `uinteger` counts only while buffered
    assert np.array_equal(rs["rng"][has, 2], gs["rng"][has, 2]), f"{what}: pcg uinteger"


def _covers_every_hand_phase(ref):
    """The workload reaches what the selects of masks_of decide: slots that are used give all-zero words
    (one and two per hand), full hands give three live words, and games end."""
    out, _ = ref
    zero_words = (out["mask"] == 0).sum(axis=2)
    live = out["terminated"] == 0
    assert (zero_words[live] == 0).any() and (zero_words[live] == 1).any() and (zero_words[live] == 2).any()
    assert out["terminated"].sum() > 20 and (out["lines"] > 0).any()


@pytest.mark.gpu
def test_rollout_masks_on_crowded_boards(cuda):
    """bb_rollout, three launches of 12 steps, against 36 chained bb_step calls and against the C oracle:
    reward bits, terminated, lines, actions, the 192-bit masks, the next action and the final state."""
    ref = _oracle("default")
    _covers_every_hand_phase(ref)
    got = _gpu_rollout(cuda, "default")
    _assert_same(ref, got, "rollout vs C oracle")
    _assert_same(_gpu_chained(cuda, "default"), got, "rollout vs chained steps")


@pytest.mark.gpu
def test_rollout_custom_reward_bits(cuda):
    """The same launches with every reward coefficient negative: float reward bits (and the rest) equal the
    C oracle's."""
    ref = _oracle("A")
    assert (ref[0]["reward"] < 0).all()
    _assert_same(ref, _gpu_rollout(cuda, "A"), "config A rollout vs C oracle")


@pytest.mark.gpu
def test_rollout_invalid_first_actions(cuda):
    """Invalid first actions in one launch of the rollout kernel: -1, 192, an occupied anchor of the unused
    slot, an anchor of a used slot.  Each gives -10 and no termination, leaves the mask (and, by the oracle's
    final state, everything else) as it was, and is followed by a legal action of the unchanged hand."""
    n, steps = 64, 2
    board = _start()[0]["board"][:n]  # fill 0.6: slots 0 and 1 used, SINGLE in slot 2
    acts = np.zeros(n, np.int32)
    for i in range(n):
        filled = [c for c in range(64) if (int(board[i]) >> c) & 1]
        acts[i] = (-1, 192, 128 + filled[i % len(filled)], 64 * (i % 2) + (i % 64))[i % 4]
    c = _oracle_env("default", n)
    mask0 = c.state()["mask"]
    ref = c.rollout(steps, acts, policy_seed=SEED, policy_step0=0)
    assert (ref["reward"][0] == -10.0).all()  # the oracle agrees that all four kinds are invalid

    env = _device_env(cuda, "default", n)
    rew = torch.zeros((steps, n), dtype=torch.float32, device=cuda)
    term = torch.ones((steps, n), dtype=torch.uint8, device=cuda)
    lines = torch.ones((steps, n), dtype=torch.uint8, device=cuda)
    aout = torch.zeros((steps, n), dtype=torch.int32, device=cuda)
    masks = torch.zeros((steps, n, 3), dtype=torch.int64, device=cuda)
    nxt = torch.zeros(n, dtype=torch.int32, device=cuda)
    env.rollout(steps, torch.from_numpy(acts).to(cuda), rew, term, lines=lines, actions_out=aout, mask_out=masks,
                next_action=nxt, policy_seed=SEED, policy_step0=0)
    env.sync()
    rew, term, lines, aout = rew.cpu().numpy(), term.cpu().numpy(), lines.cpu().numpy(), aout.cpu().numpy()
    masks = masks.cpu().numpy().view(np.uint64)
    assert (rew[0] == -10.0).all() and not term[0].any() and not lines[0].any()
    assert np.array_equal(aout[0], acts)
    assert np.array_equal(masks[0], mask0)  # the step left hand and board alone
    a1 = aout[1]
    assert np.array_equal(a1, c.random_actions(mask0, SEED, 1))
    assert ((masks[0][np.arange(n), a1 >> 6] >> (a1 & 63).astype(np.uint64)) & np.uint64(1)).all()  # legal
    for k, g in (("reward", rew), ("terminated", term), ("lines", lines), ("actions", aout), ("mask", masks)):
        a, b = (ref[k].view(np.uint32), g.view(np.uint32)) if k == "reward" else (ref[k], g)
        assert np.array_equal(a, b), k
    assert np.array_equal(nxt.cpu().numpy(), ref["next_action"])
    gs, cs = env.state(), c.state()
    for k in ("board", "hand", "score", "combo", "max_combo", "moves", "lines", "blocks", "prev_holes",
              "prev_center"):
        assert np.array_equal(gs[k], cs[k]), f"state {k}"
    assert np.array_equal(gs["rng"][:, :2], cs["rng"][:, :2])
    env.close()
    c.close()
