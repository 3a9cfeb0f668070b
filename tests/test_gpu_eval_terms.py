"""The shape terms and the search with them on the MI355X (board_terms_kernel / plan_ext_kernel in
csrc/bb_lookahead.hip: bb_board_terms(_pos), bb_plan_actions_ext(_pos)).

* board_terms: against the cell-by-cell reference of tests/_eval_terms_ref.py on the crafted families; against the
  host backend on 4,099 random boards and above the kernel's grid cap; n = 1, 63, 64, 65; guard words behind the
  output; the handle form against the _pos form on a snapshot.
* plan_actions_ext: against the reference search on the 92 positions (depth 1-2, and depth 3 on the small trees);
  against the host backend at n = 1, 5, 67 (depth 1-3) and on 1,031 mid-game positions at depth 3; zero shape
  weights against the existing plan_actions_each; above the plan grid cap against per-set calls gathered; a graph
  captured once and replayed after rows and boards were rewritten in place; stride 0 against replicated rows; the
  handle form; tensors on the wrong side.
* HandPlanAgent with shape weights and evaluate_population with 12-wide dicts, GPU against host.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _eval_terms_ref as E

pytestmark = pytest.mark.gpu

KEYS = ("action", "value", "plan", "leaves")
CPU = torch.device("cpu")
N_MID = 1031
PLAN_MAX_GRID = 1 << 14          # kPlanMaxGrid of csrc/bb_lookahead.hip
TERMS_MAX_LANES = (1 << 10) * 256  # kTermsMaxGrid * kTermsBlock
NAMES = list(E.SETS)


@pytest.fixture(scope="module")
def ref():
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return R.reference()


def _i64(boards):
    return torch.from_numpy(np.asarray(boards, np.uint64).view(np.int64).copy())


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
    st = env.state()
    return (torch.from_numpy(st["board"].view(np.int64).copy()).to(env.device),
            torch.from_numpy(st["hand"].view(np.int32).copy()).to(env.device),
            torch.from_numpy(st["combo"].copy()).to(env.device))


def _assert_same(got, want, what):
    for k in want:
        g, x = torch.as_tensor(got[k]).cpu(), torch.as_tensor(want[k]).cpu()
        bad = torch.nonzero((g != x).reshape(g.shape[0], -1).any(dim=1)).flatten()[:4]
        assert bad.numel() == 0, (what, k, bad.tolist(), g[bad].tolist(), x[bad].tolist())


def _ext(cols, rows, depth):
    from runtime import kernels as K

    return K.plan_actions_ext(cols[0], cols[1], rows, depth, combo=cols[2], want_plan=True, want_leaves=True)


def _dealt_rows(n, dev, shift=0, cap=None):
    """(rows int32 [n, 12], set index [n]): position i takes set (i + shift) % 7, or (i + i // cap) % 7."""
    from runtime import kernels as K

    i = np.arange(n)
    which = (i + shift) % len(NAMES) if cap is None else (i + i // cap) % len(NAMES)
    table = K.eval_rows([E.SETS[k] for k in NAMES], device=dev)
    return table[torch.as_tensor(which, device=dev)].contiguous(), which


def _gathered(per_set, which):
    sel = torch.as_tensor(which)
    return {k: torch.stack([r[k].cpu() for r in per_set])[sel, torch.arange(len(which))] for k in KEYS}


# ---------------------------------------------------------------------------------------------------------------
# board_terms
# ---------------------------------------------------------------------------------------------------------------
def test_board_terms_equal_the_cell_reference_on_the_crafted_families(cuda):
    from runtime import kernels as K

    boards, want, where = E.reference_terms()
    got = K.board_terms(_i64(boards).to(cuda)).cpu().numpy()
    for fam, sl in where.items():
        bad = np.nonzero((got[sl] != want[sl]).any(axis=1))[0][:4]
        assert bad.size == 0, (fam, [hex(int(b)) for b in boards[sl][bad]], got[sl][bad], want[sl][bad])
    assert got[where["basic"]].tolist() == [[32, 36, 64, 37], [0, 0, 0, 0], [128, 0, 0, 5]]
    assert (got[where["window3x3"]][:, 1] == 1).all() and (got[where["window1x5"]][:, 2] == 1).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099, TERMS_MAX_LANES + 3])
def test_board_terms_equal_the_host_backend_with_guard_words(cuda, ref, n):
    from runtime import kernels as K

    boards = _i64(E.random_boards(n, 77 + n))
    want = K.board_terms(boards)
    buf = torch.full((n * 4 + 8,), -99, dtype=torch.int32, device=cuda)
    K.board_terms(boards.to(cuda), out=buf[:n * 4].view(n, 4))
    assert torch.equal(buf[:n * 4].view(n, 4).cpu(), want)
    assert bool((buf[n * 4:] == -99).all())
    assert want[0].tolist() == [32, 36, 64, 37] and (n == 1 or want[-1].tolist() == [0, 0, 0, 0])  # empty .. full


def test_board_terms_handle_form_equals_pos_form(cuda):
    from runtime import kernels as K

    env = _rolled(67, 30, 11, cuda)
    board = _columns(env)[0]
    got = torch.full((67, 4), -5, dtype=torch.int32, device=cuda)
    env.board_terms(got)
    assert torch.equal(got, K.board_terms(board)) and int(got[:, 0].max()) > 32
    assert K.board_terms(torch.zeros(0, dtype=torch.int64, device=cuda)).shape == (0, 4)
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# plan_actions_ext
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_ext_equals_the_reference_search(cuda, ref, depth):
    from runtime import kernels as K

    idx, want = E.reference_plans(depth, depth < 3)  # depth 3: the trees of at most 20,000 leaves
    cols = tuple(t.to(cuda) for t in R.tensors(ref, CPU, idx)[:3])
    for name, w in E.SETS.items():
        _assert_same(_ext(cols, K.eval_rows(w, device=cuda), depth), want[name], f"{name} depth {depth}")


@pytest.mark.parametrize("n", [1, 5, 67])
def test_ext_equals_host_backend_and_handle_equals_pos(cuda, ref, n):
    from runtime.device_env import DeviceEnvBatch

    crafted = sorted(ref["names"].values())
    idx = np.array((crafted + [i for i in range(ref["n"]) if i not in crafted])[:n])
    cpu_cols = R.tensors(ref, CPU, idx)[:3]
    cols = tuple(t.to(cuda) for t in cpu_cols)
    rows, _ = _dealt_rows(n, CPU, shift=5)  # n = 1 plays `all`
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    before = env.state()
    for depth in (1, 2, 3):
        want = _ext(cpu_cols, rows, depth)
        _assert_same(_ext(cols, rows.to(cuda), depth), want, f"_pos n={n} depth={depth}")
        o = _outputs(n, cuda)
        env.plan_actions_ext(o["action"], rows.to(cuda), depth, value=o["value"], plan=o["plan"], leaves=o["leaves"])
        _assert_same(o, want, f"handle n={n} depth={depth}")
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before), "the handle form changed the state"
    env.close()


@pytest.fixture(scope="module")
def mid(cuda):
    env = _rolled(N_MID, 40, 7, cuda)
    yield env, _columns(env)
    env.close()


@pytest.mark.parametrize("name", ["all", "mixed"])
def test_mid_game_ext_equals_host_backend(cuda, ref, mid, name):
    from runtime import kernels as K

    _, cols = mid
    rows = K.eval_rows(E.SETS[name])
    want = _ext(tuple(t.cpu() for t in cols), rows, 3)
    _assert_same(_ext(cols, rows.to(cuda), 3), want, f"mid-game depth 3 {name}")
    assert int(want["leaves"].max()) > 100_000 and bool((want["plan"][:, 2] >= 0).any())


def test_zero_shape_weights_equal_plan_actions_each_and_stride0_equals_replicated(cuda, mid):
    from runtime import kernels as K

    _, cols = mid
    for base in (E.SETS["zero4"], {k: v for k, v in E.SETS["mixed"].items() if k in R.DEFAULT_WEIGHTS}):
        want = K.plan_actions_each(cols[0], cols[1], K.weight_rows(base, n=N_MID, device=cuda), 3, combo=cols[2],
                                   want_plan=True, want_leaves=True)
        _assert_same(_ext(cols, K.eval_rows(base, device=cuda), 3), want, "zero shape weights, shared row")
        _assert_same(_ext(cols, K.eval_rows(base, n=N_MID, device=cuda), 3), want, "zero shape weights, own rows")
    shared = _ext(cols, K.eval_rows(E.SETS["all"], device=cuda), 3)
    _assert_same(_ext(cols, K.eval_rows(E.SETS["all"], n=N_MID, device=cuda), 3), shared, "stride 0 = stride 1")
    assert not torch.equal(shared["action"], want["action"])


def test_ext_above_the_grid_cap_reads_its_own_row(cuda):
    from runtime import kernels as K

    n = PLAN_MAX_GRID + 3
    env = _rolled(n, 25, 1000, cuda)
    cols = _columns(env)
    rows, which = _dealt_rows(n, cuda, cap=PLAN_MAX_GRID)
    assert (which[PLAN_MAX_GRID:] != which[:n - PLAN_MAX_GRID]).all()
    per_set = [_ext(cols, K.eval_rows(E.SETS[k], device=cuda), 2) for k in NAMES]
    got = _ext(cols, rows, 2)
    _assert_same(got, _gathered(per_set, which), "ext above the grid cap, depth 2")
    wrapped = torch.arange(PLAN_MAX_GRID, n)  # under the row of position i - cap the values would have differed
    by_set = torch.stack([u["value"].cpu() for u in per_set])
    assert not torch.equal(got["value"].cpu()[wrapped], by_set[torch.as_tensor(which[:n - PLAN_MAX_GRID]), wrapped])
    env.close()


def test_graph_replay_reads_rows_and_boards_of_the_moment(cuda, mid):
    from runtime import kernels as K

    _, (board, hand, combo) = mid
    first, _ = _dealt_rows(N_MID, cuda)
    second, _ = _dealt_rows(N_MID, cuda, shift=3)
    board2 = torch.roll(board, 1)
    eager = [_ext((b, hand, combo), r, 3) for b, r in ((board, first), (board2, second))]
    assert not torch.equal(eager[0]["action"], eager[1]["action"])
    rows, live = first.clone(), board.clone()
    o = _outputs(N_MID, cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # captured from the first call made with these buffers
        K.plan_actions_ext(live, hand, rows, 3, combo=combo, **{k: o[k] for k in KEYS})
    for want, new in zip(eager, (None, (board2, second))):
        if new is not None:
            live.copy_(new[0])
            rows.copy_(new[1])
        for t in o.values():
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(o, want, "graph replay")


def test_no_legal_action_and_tensors_on_the_wrong_side(cuda, ref, mid):
    from _weights_each import no_action_positions
    from runtime import kernels as K
    from runtime.lib import BBNativeError

    board, hand = no_action_positions(ref)
    rows, _ = _dealt_rows(8, cuda)
    for depth in (1, 2, 3):
        got = K.plan_actions_ext(board.to(cuda), hand.to(cuda), rows, depth, want_plan=True, want_leaves=True)
        assert bool((got["action"] == 0).all()) and bool((got["value"] == R.INT64_MIN).all())
        assert bool((got["plan"] == -1).all()) and bool((got["leaves"] == 0).all())
    env, (board, hand, combo) = mid
    host_rows = K.eval_rows(E.SETS["all"])
    out = torch.zeros(N_MID, dtype=torch.int32, device=cuda)
    with pytest.raises(BBNativeError, match="rows must be"):
        env.plan_actions_ext(out, host_rows, 3)
    with pytest.raises(BBNativeError, match="action must be"):
        env.plan_actions_ext(out.cpu(), host_rows.to(cuda), 3)
    with pytest.raises(BBNativeError, match="rows must be"):
        K.plan_actions_ext(board, hand, host_rows, 3, combo=combo)
    with pytest.raises(BBNativeError, match="rows must be"):
        K.plan_actions_ext(board.cpu(), hand.cpu(), host_rows.to(cuda), 3, combo=combo.cpu())
    with pytest.raises(BBNativeError, match=r"\[1, 12\] or \[1031, 12\]"):
        K.plan_actions_ext(board, hand, K.eval_rows(E.SETS["all"], n=5, device=cuda), 3, combo=combo)


# ---------------------------------------------------------------------------------------------------------------
# agents
# ---------------------------------------------------------------------------------------------------------------
def test_hand_plan_agent_with_shape_weights_plays_what_the_host_backend_plays(cuda, ref):
    from agents.greedy import HandPlanAgent
    from runtime.device_env import DeviceEnvBatch

    played = {}
    for dev in (cuda, CPU):
        agent = HandPlanAgent(E.SETS["all"], depth=3, device=dev)
        env = DeviceEnvBatch(8, [900 + i for i in range(8)], autoreset=False, device=dev)
        env.reset()
        out = torch.zeros(8, dtype=torch.int32, device=dev)
        moves = []
        for _ in range(12):
            agent.act_env(env, out)
            moves.append(out.cpu().clone())
            env.step(out)
        played[dev.type] = (torch.stack(moves), env.state()["score"].copy())
        env.close()
    assert torch.equal(played["cuda"][0], played["cpu"][0]) and np.array_equal(played["cuda"][1], played["cpu"][1])


def test_evaluate_population_with_shape_weights_gpu_equals_host(cuda, ref):
    from evaluation.tune import evaluate_population

    sets = [E.SETS[k] for k in ("zero4", "per", "all", "mixed")]
    got = evaluate_population(sets, 3, 30, 5, depth=3, device=cuda)
    want = evaluate_population(sets, 3, 30, 5, depth=3, device="cpu")
    assert got.shape == (4, 3) and torch.equal(got, want)
    assert not torch.equal(got[0], got[2])
