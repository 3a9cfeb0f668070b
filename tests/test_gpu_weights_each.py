"""One row of weights per position on the MI355X (greedy_each_kernel / plan_each_kernel in csrc/bb_lookahead.hip:
bb_greedy_actions_each(_pos), bb_plan_actions_each(_pos)).

* Against the host backend's _each calls (which tests/test_weights_each_host.py holds to the uniform calls), all
  outputs, at n = 1, 5 and 67 of the reference set with mixed rows, stateless and handle form, depth 1-3, and at
  n = 1,031 mid-game positions at depth 3.
* Above the grid caps (16,384 workgroups for the plan kernel, 32,768 for the greedy kernel), where a workgroup takes a
  second position: the rows are dealt so that position i + cap has another row than position i, which a row load
  hoisted out of the position loop gets wrong.  Against the uniform HIP calls gathered by set.
* All rows equal against the uniform HIP call; a graph replay that sees the rows overwritten in place; rows at the
  ends of int32 and positions without a legal action; tensors on the wrong side refused.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
from _weights_each import KEYS, SETS, gathered, mixed_rows, no_action_positions

pytestmark = pytest.mark.gpu

N_MID = 1031
PLAN_MAX_GRID = 1 << 14  # kPlanMaxGrid of csrc/bb_lookahead.hip
LOOK_MAX_GRID = 1 << 15  # kLookMaxGrid


@pytest.fixture(scope="module")
def ref():
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return R.reference()


def _outputs(n, dev):
    return {"action": torch.full((n,), -7, dtype=torch.int32, device=dev),
            "value": torch.full((n,), 5, dtype=torch.int64, device=dev),
            "plan": torch.full((n, 3), -7, dtype=torch.int32, device=dev),
            "leaves": torch.full((n,), -7, dtype=torch.int32, device=dev)}


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


def _columns(env):
    """The env's positions as (board, hand, combo) tensors on its device."""
    st = env.state()
    return (torch.from_numpy(st["board"].view(np.int64).copy()).to(env.device),
            torch.from_numpy(st["hand"].view(np.int32).copy()).to(env.device),
            torch.from_numpy(st["combo"].copy()).to(env.device))


def _assert_same(got, want, what):
    for k in want:
        g, x = got[k].cpu(), want[k].cpu()
        bad = torch.nonzero((g != x).reshape(g.shape[0], -1).any(dim=1)).flatten()[:4]
        assert bad.numel() == 0, (what, k, bad.tolist(), g[bad].tolist(), x[bad].tolist())


@pytest.mark.parametrize("n", [1, 5, 67])
def test_each_equals_host_backend_on_the_reference_set(cuda, ref, n):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    crafted = sorted(ref["names"].values())
    idx = np.array((crafted + [i for i in range(ref["n"]) if i not in crafted])[:n])
    rows, _ = mixed_rows(n, shift=1)  # n = 1 plays the defaults
    cpu_cols = R.tensors(ref, torch.device("cpu"), idx)[:3]
    board, hand, combo = (t.to(cuda) for t in cpu_cols)
    drows = rows.to(cuda)
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    before = env.state()
    for depth in (1, 2, 3):
        want = K.plan_actions_each(cpu_cols[0], cpu_cols[1], rows, depth, combo=cpu_cols[2], want_plan=True,
                                   want_leaves=True)
        got = K.plan_actions_each(board, hand, drows, depth, combo=combo, want_plan=True, want_leaves=True)
        _assert_same(got, want, f"_pos n={n} depth={depth}")
        o = _outputs(n, cuda)
        env.plan_actions_each(o["action"], drows, depth, value=o["value"], plan=o["plan"], leaves=o["leaves"])
        _assert_same(o, want, f"handle n={n} depth={depth}")
    want = dict(zip(("action", "value"), K.greedy_actions_each(cpu_cols[0], cpu_cols[1], rows, combo=cpu_cols[2])))
    got = dict(zip(("action", "value"), K.greedy_actions_each(board, hand, drows, combo=combo)))
    _assert_same(got, want, f"greedy _pos n={n}")
    o = _outputs(n, cuda)
    env.greedy_actions_each(o["action"], drows, value=o["value"])
    _assert_same({k: o[k] for k in want}, want, f"greedy handle n={n}")
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


@pytest.fixture(scope="module")
def mid(cuda):
    env = _rolled(N_MID, 40, 7, cuda)
    yield env, _columns(env)
    env.close()


def test_mid_game_each_equals_host_backend(cuda, ref, mid):
    from runtime import kernels as K

    env, (board, hand, combo) = mid
    rows, _ = mixed_rows(N_MID)
    want = K.plan_actions_each(board.cpu(), hand.cpu(), rows, 3, combo=combo.cpu(), want_plan=True, want_leaves=True)
    o = _outputs(N_MID, cuda)
    env.plan_actions_each(o["action"], rows.to(cuda), 3, value=o["value"], plan=o["plan"], leaves=o["leaves"])
    _assert_same(o, want, "mid-game depth 3")
    assert int(want["leaves"].max()) > 100_000 and bool((want["plan"][:, 2] >= 0).any())


def _striding_rows(n, cap, dev):
    """Rows dealt so that the positions one workgroup takes (i, i + cap) have different rows."""
    from runtime import kernels as K

    i = np.arange(n)
    which = (i + i // cap) % len(SETS)
    assert (which[cap:] != which[:n - cap]).all()
    table = K.weight_rows(SETS, device=dev)
    return table[torch.as_tensor(which, device=dev)].contiguous(), which


def _assert_wrapped_differ(got, uniform, which, cap):
    """Not vacuous: under the row of position i - cap (what a hoisted load would use) the wrapped positions
    would have had other values."""
    n = len(which)
    wrapped = torch.arange(cap, n)
    by_set = torch.stack([u["value"].cpu() for u in uniform])
    assert not torch.equal(got["value"].cpu()[wrapped], by_set[torch.as_tensor(which[:n - cap]), wrapped])


def test_plan_each_above_the_grid_cap_reads_its_own_row(cuda):
    from runtime import kernels as K

    n = PLAN_MAX_GRID + 3
    env = _rolled(n, 25, 1000, cuda)
    board, hand, combo = _columns(env)
    rows, which = _striding_rows(n, PLAN_MAX_GRID, cuda)
    uniform = [K.plan_actions(board, hand, w, 2, combo=combo, want_plan=True, want_leaves=True) for w in SETS]
    got = K.plan_actions_each(board, hand, rows, 2, combo=combo, want_plan=True, want_leaves=True)
    _assert_same(got, gathered(uniform, which), "plan_each above the grid cap, depth 2")
    _assert_wrapped_differ(got, uniform, which, PLAN_MAX_GRID)
    env.close()


def test_greedy_each_above_the_grid_cap_reads_its_own_row(cuda):
    from runtime import kernels as K

    n = LOOK_MAX_GRID + 3
    env = _rolled(n, 25, 5000, cuda)
    board, hand, combo = _columns(env)
    rows, which = _striding_rows(n, LOOK_MAX_GRID, cuda)
    uniform = [dict(zip(("action", "value"), K.greedy_actions(board, hand, w, combo=combo))) for w in SETS]
    got = dict(zip(("action", "value"), K.greedy_actions_each(board, hand, rows, combo=combo)))
    _assert_same(got, gathered(uniform, which), "greedy_each above the grid cap")
    _assert_wrapped_differ(got, uniform, which, LOOK_MAX_GRID)
    env.close()


def test_equal_rows_equal_the_uniform_kernel(cuda):
    from runtime import kernels as K

    n = 4099
    env = _rolled(n, 40, 300, cuda)
    board, hand, combo = _columns(env)
    for w in (SETS[1], SETS[3]):
        rows = K.weight_rows(w, n=n, device=cuda)
        want = K.plan_actions(board, hand, w, 3, combo=combo, want_plan=True, want_leaves=True)
        got = K.plan_actions_each(board, hand, rows, 3, combo=combo, want_plan=True, want_leaves=True)
        _assert_same(got, want, "equal rows, depth 3")
        want = dict(zip(("action", "value"), K.greedy_actions(board, hand, w, combo=combo)))
        got = dict(zip(("action", "value"), K.greedy_actions_each(board, hand, rows, combo=combo)))
        _assert_same(got, want, "equal rows, greedy")
    env.close()


def test_graph_replay_reads_the_rows_of_the_moment(cuda, mid):
    """One captured launch, the rows overwritten in place between two replays, no re-capture: the tuner's
    per-generation reuse relies on it."""
    from runtime import kernels as K

    _, (board, hand, combo) = mid
    first, _ = mixed_rows(N_MID, cuda)
    second, _ = mixed_rows(N_MID, cuda, shift=1)
    eager = [K.plan_actions_each(board, hand, r, 3, combo=combo, want_plan=True, want_leaves=True)
             for r in (first, second)]
    assert not torch.equal(eager[0]["action"], eager[1]["action"])
    rows = first.clone()
    o = _outputs(N_MID, cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # captured from the first call made with these buffers
        K.plan_actions_each(board, hand, rows, 3, combo=combo, **{k: o[k] for k in KEYS})
    for want, new_rows in zip(eager, (None, second)):
        if new_rows is not None:
            rows.copy_(new_rows)
        for t in o.values():
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(o, want, "graph replay")


def test_extreme_rows_and_positions_without_a_legal_action(cuda, ref, mid):
    from runtime import kernels as K

    board, hand = no_action_positions(ref)
    rows, _ = mixed_rows(8)
    for depth in (1, 2, 3):
        got = K.plan_actions_each(board.to(cuda), hand.to(cuda), rows.to(cuda), depth, want_plan=True,
                                  want_leaves=True)
        assert bool((got["action"] == 0).all()) and bool((got["value"] == R.INT64_MIN).all())
        assert bool((got["plan"] == -1).all()) and bool((got["leaves"] == 0).all())
    act, val = K.greedy_actions_each(board.to(cuda), hand.to(cuda), rows.to(cuda))
    assert bool((act == 0).all()) and bool((val == R.INT64_MIN).all())

    # every row at the ends of int32, signs alternating by position, on mid-game positions; NULL optional outputs
    _, (mb, mh, mc) = mid
    n = 67
    ext = K.weight_rows([SETS[3] if i % 2 == 0 else {k: -v for k, v in SETS[3].items()} for i in range(n)])
    cols = (mb[:n].contiguous(), mh[:n].contiguous(), mc[:n].contiguous())
    want = K.plan_actions_each(cols[0].cpu(), cols[1].cpu(), ext, 3, combo=cols[2].cpu(), want_plan=True,
                               want_leaves=True)
    got = K.plan_actions_each(cols[0], cols[1], ext.to(cuda), 3, combo=cols[2], want_plan=True, want_leaves=True)
    _assert_same(got, want, "extreme rows, depth 3")
    alone = K.plan_actions_each(cols[0], cols[1], ext.to(cuda), 3, combo=cols[2], want_value=False)
    assert set(alone) == {"action"} and torch.equal(alone["action"], got["action"])
    ga, gv = K.greedy_actions_each(cols[0], cols[1], ext.to(cuda), combo=cols[2], want_value=False)
    assert gv is None and torch.equal(ga.cpu(), K.greedy_actions_each(cols[0].cpu(), cols[1].cpu(), ext,
                                                                       combo=cols[2].cpu())[0])


def test_tensors_on_the_wrong_side_are_refused(cuda, mid):
    """As the uniform handle forms: a handle takes tensors of its own device only -- a HIP env no host rows or
    outputs, a host env no device rows, the stateless call no rows away from its positions."""
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch
    from runtime.lib import BBNativeError

    env, (board, hand, combo) = mid
    rows, _ = mixed_rows(N_MID)
    out = torch.zeros(N_MID, dtype=torch.int32, device=cuda)
    with pytest.raises(BBNativeError, match="rows must be"):
        env.plan_actions_each(out, rows, 3)
    with pytest.raises(BBNativeError, match="rows must be"):
        env.greedy_actions_each(out, rows)
    with pytest.raises(BBNativeError, match="action must be"):
        env.plan_actions_each(out.cpu(), rows.to(cuda), 3)
    with pytest.raises(BBNativeError, match="rows must be"):
        K.plan_actions_each(board, hand, rows, 3, combo=combo)
    host = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    host.reset()
    with pytest.raises(BBNativeError, match="rows must be"):
        host.plan_actions_each(torch.zeros(4, dtype=torch.int32), rows[:4].to(cuda), 3)
    host.close()
    if torch.cuda.device_count() > 1:  # a handle on another device than the rows
        other = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cuda:1")
        with pytest.raises(BBNativeError, match="action must be"):
            other.plan_actions_each(out[:4].contiguous(), rows[:4].to(cuda), 3)
        other.close()
