"""The env waves' draw gate (rollout_async_kernel, BB_ASYNC_DGATE) against chained bb_step calls.

An env whose move used its hand's last piece waits, "wanting a draw", until its wave opens the draw block:
when enough of the wave's runnable envs want one, when the gate stayed closed for its limit of iterations,
or when no env moved.  Only the order in which a wave's envs advance may change: every per-step output
(reward bits, terminated, lines, applied action, post-step mask), the final state and the next policy action
must equal what T chained bb_step calls give (bb_step is pinned to the CPU oracle by
test_gpu_env_parity.py).  The shapes are the smallest at which a gate can go wrong: a few lanes (the share
rule can never hold a wave together), wave and workgroup edges, launches shorter than the gate's period
starting at every hand phase, a trajectory cut into launches that end on draws, and crowded boards whose
long searches make envs re-join out of phase.  After every launch bb_sync must succeed: no wave left through
an iteration cap.
"""
import numpy as np
import pytest
import torch

from _crowded import crowded_setup

pytestmark = pytest.mark.gpu

SEED = 0xB10C


def _fresh(n, cuda):
    """n envs after reset (seeds 42 + i) and the policy's first action."""
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(n, seeds=[42 + i for i in range(n)], device=cuda)
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64, device=cuda)
    env.obs(mask_bits=mb)
    a0 = torch.zeros(n, dtype=torch.int32, device=cuda)
    env.random_actions(mb, a0, seed=SEED, step=0)
    return env, a0


_CROWDED = {}


def _crowded(n, cuda, fill=0.9):
    """n envs on crowded boards whose first move uses the hand's last slot (tests/_crowded.py)."""
    from runtime.device_env import DeviceEnvBatch

    if (n, fill) not in _CROWDED:
        state, acts, _ = crowded_setup(fill, n)
        _CROWDED[(n, fill)] = (state, acts)
    state, acts = _CROWDED[(n, fill)]
    env = DeviceEnvBatch(n, seeds=[5000 + i for i in range(n)], device=cuda)
    env.set_state(**state)
    return env, torch.from_numpy(acts).to(cuda)


def _warm(env, a, warm):
    nxt = torch.zeros_like(a)
    for t in range(warm):
        env.step(a, next_action=nxt, policy_seed=SEED, policy_step=t + 1)
        a, nxt = nxt, a
    return a, nxt


def _finish(env, out, a):
    env.sync()  # raises if a wave left through an iteration cap
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["next_action"] = a.cpu().numpy()
    st = env.state()
    env.close()
    return out, st


def _chained(make, n, steps, cuda, warm=0):
    env, a = make(n, cuda)
    a, nxt = _warm(env, a, warm)
    rew, term, lines, acts, masks = [], [], [], [], []
    mb = torch.zeros((n, 3), dtype=torch.int64, device=cuda)
    for t in range(steps):
        acts.append(a.clone())
        env.step(a, next_action=nxt, want_lines=True, policy_seed=SEED, policy_step=warm + t + 1, mask_out=mb)
        rew.append(env.reward.clone())
        term.append(env.terminated.clone())
        lines.append(env.lines.clone())
        masks.append(mb.clone())
        a, nxt = nxt, a
    out = {"reward": torch.stack(rew), "terminated": torch.stack(term), "lines": torch.stack(lines),
           "actions": torch.stack(acts), "mask": torch.stack(masks)}
    return _finish(env, out, a)


def _rollout(make, n, steps, cuda, warm=0, splits=()):
    env, a = make(n, cuda)
    a, nxt = _warm(env, a, warm)
    out = {"reward": torch.zeros((steps, n), dtype=torch.float32, device=cuda),
           "terminated": torch.zeros((steps, n), dtype=torch.uint8, device=cuda),
           "lines": torch.zeros((steps, n), dtype=torch.uint8, device=cuda),
           "actions": torch.zeros((steps, n), dtype=torch.int32, device=cuda),
           "mask": torch.zeros((steps, n, 3), dtype=torch.int64, device=cuda)}
    bounds = [0, *splits, steps]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        env.rollout(hi - lo, a, out["reward"][lo:hi], out["terminated"][lo:hi], lines=out["lines"][lo:hi],
                    actions_out=out["actions"][lo:hi], mask_out=out["mask"][lo:hi], next_action=nxt,
                    policy_seed=SEED, policy_step0=warm + lo)
        a, nxt = nxt, a
        env.sync()  # each launch on its own: none may leave through a cap
    return _finish(env, out, a)


def _assert_same(ref, got):
    (ro, rs), (go, gs) = ref, got
    for k in ro:
        if k == "reward":
            assert np.array_equal(ro[k].view(np.uint32), go[k].view(np.uint32)), k
        else:
            assert np.array_equal(ro[k], go[k]), k
    for k in rs:
        if k == "rng":  # numpy's `uinteger` is meaningful only while has_uint32 (hand bit 22) is set
            assert np.array_equal(rs[k][:, :2], gs[k][:, :2]), "state rng"
            has = ((rs["hand"] >> 22) & 1).astype(bool)
            assert np.array_equal(rs[k][has, 2], gs[k][has, 2]), "state rng uinteger"
        else:
            assert np.array_equal(rs[k], gs[k]), f"state {k}"


@pytest.mark.parametrize("n", [1, 2, 3])
def test_few_lanes(cuda, n):
    """One to three envs: two wanting lanes of three are the only way to a half share, so mostly the
    closed-streak limit and the no-env-moved rule open the gate."""
    _assert_same(_chained(_fresh, n, 40, cuda), _rollout(_fresh, n, 40, cuda))


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_workgroup_edges(cuda, n):
    """A wave short of one lane, a full wave, a second wave of one env, a second workgroup of one env."""
    _assert_same(_chained(_fresh, n, 30, cuda), _rollout(_fresh, n, 30, cuda))


@pytest.mark.parametrize("warm", [0, 1, 2])
@pytest.mark.parametrize("steps", [2, 3, 4, 7])
def test_short_launches_at_every_hand_phase(cuda, steps, warm):
    """Launches shorter than the gate's period (a hand lasts three moves), started with three, two and one
    piece left: the first draw falls on the launch's third, second and first step, the last launches end
    while envs still want one."""
    _assert_same(_chained(_fresh, 65, steps, cuda, warm=warm), _rollout(_fresh, 65, steps, cuda, warm=warm))


def test_launches_that_end_on_a_draw(cuda):
    """64 steps as consecutive launches of 2, 3, 5, 7, 11, 13, 17 and 6 steps equal one launch and the chained
    steps: hand, stream and mask carry across launches whatever hand phase a launch ends on."""
    ref = _chained(_fresh, 65, 64, cuda)
    _assert_same(ref, _rollout(_fresh, 65, 64, cuda))
    _assert_same(ref, _rollout(_fresh, 65, 64, cuda, splits=(2, 5, 10, 17, 28, 41, 58)))


def test_crowded_boards_rejoin_out_of_phase(cuda):
    """Boards filled to 0.9: most first hands are posted and searched for many attempts, episodes end and
    reset, so the envs of a wave keep falling out of the wave's hand phase."""
    ref = _chained(_crowded, 257, 40, cuda)
    assert ref[0]["terminated"].any()
    _assert_same(ref, _rollout(_crowded, 257, 40, cuda))
