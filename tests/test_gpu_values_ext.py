"""bb_plan_values_ext / bb_refill_values_ext on the MI355X (plan_values_ext_kernel / refill_values_ext_kernel in
csrc/bb_lookahead.hip).

* plan_values_ext: against the reference of tests/_values_ext_ref.py on the 92 positions under the seven weight sets
  (depth 1-2, and depth 3 on the small trees); against the host backend on the whole set at depth 1-3 with the sets
  interleaved, all four outputs; 16,387 positions (kPlanMaxGrid + 3) at depth 2 with rows dealt so that i and
  i + cap differ, against per-set calls; rows with zero shape weights and shaped rows in one launch, each side held to
  the call it must equal; a graph captured once and replayed after rows, boards and outputs were rewritten in place;
  the handle form against the _pos form on a snapshot; tensors on the wrong device.
* refill_values_ext: against the reference; 129 boards x 128 deals (kRefillMaxGrid + 128 pairs) at depth 1 with
  per-board rows against the host backend; both branch sides; graph replay; the handle form.
* TwoHandShapeAgent: the host backend's moves for 4 games x 30 moves with 4 candidates and 4 deals.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _refill_values_ref as RV
import _values_ext_ref as X

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
PV_KEYS = ("q", "rest", "leaves", "safe")
RV_KEYS = ("hand", "value", "attempts")
PLAN_MAX_GRID = 1 << 14    # kPlanMaxGrid of csrc/bb_lookahead.hip
REFILL_MAX_GRID = 1 << 14  # kRefillMaxGrid
NAMES = X.NAMES
N_MID = 259


@pytest.fixture(scope="module")
def ref():
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return R.reference()


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


@pytest.fixture(scope="module")
def mid(cuda):
    env = _rolled(N_MID, 40, 7, cuda)
    yield env, _columns(env)
    env.close()


def _same(got, want, keys, what):
    for k in keys:
        g, x = got[k].cpu(), want[k].cpu()
        assert torch.equal(g, x), (what, k, torch.nonzero(g != x)[:4].tolist())


def _pv(cols, rows, depth, **kw):
    from runtime import kernels as K

    return K.plan_values_ext(cols[0], cols[1], rows, depth, combo=cols[2], **kw)


def _dealt_rows(n, dev, shift=0, cap=None):
    """(rows int32 [n, 12], set index [n]): position i takes set (i + shift) % 7, or (i + i // cap) % 7."""
    from runtime import kernels as K

    i = np.arange(n)
    which = (i + shift) % len(NAMES) if cap is None else (i + i // cap) % len(NAMES)
    table = K.eval_rows([X.SETS[k] for k in NAMES], device=dev)
    return table[torch.as_tensor(which, device=dev)].contiguous(), which


def _gathered(per_set, which, keys):
    sel = torch.as_tensor(which)
    return {k: torch.stack([r[k].cpu() for r in per_set])[sel, torch.arange(len(which))] for k in keys}


def _base(w):
    return {k: v for k, v in w.items() if k in R.DEFAULT_WEIGHTS}


# ---------------------------------------------------------------------------------------------------------------
# plan_values_ext
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_plan_values_ext_equals_the_reference(cuda, ref, depth):
    from runtime import kernels as K

    idx, want = X.reference_values(depth, depth < 3)  # depth 3: the trees of at most 20,000 leaves
    cols = tuple(t.to(cuda) for t in R.tensors(ref, CPU, idx)[:3])
    for name, w in X.SETS.items():
        X.check(_pv(cols, K.eval_rows(w, device=cuda), depth), want, name, what=f"depth {depth}")


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_plan_values_ext_equals_the_host_backend_on_the_whole_set(cuda, ref, depth):
    cpu_cols = R.tensors(ref, CPU)[:3]
    rows, which = _dealt_rows(ref["n"], CPU, shift=depth)
    want = _pv(cpu_cols, rows, depth)
    got = _pv(tuple(t.to(cuda) for t in cpu_cols), rows.to(cuda), depth)
    _same(got, want, PV_KEYS, f"whole set, depth {depth}")
    assert int(want["leaves"].sum(dim=1).max()) > (100_000 if depth == 3 else 100)


def test_plan_values_ext_above_the_grid_cap_reads_its_own_row(cuda):
    from runtime import kernels as K

    n = PLAN_MAX_GRID + 3
    env = _rolled(n, 25, 1000, cuda)
    cols = _columns(env)
    rows, which = _dealt_rows(n, cuda, cap=PLAN_MAX_GRID)
    assert (which[PLAN_MAX_GRID:] != which[:n - PLAN_MAX_GRID]).all()
    got = _pv(cols, rows, 2)
    got = {k: v.cpu() for k, v in got.items()}
    qs = []
    for j, name in enumerate(NAMES):  # per-set calls, one at a time: each holds [n, 192] outputs
        one = _pv(cols, K.eval_rows(X.SETS[name], device=cuda), 2)
        sel = torch.as_tensor(which == j)
        for k in PV_KEYS:
            assert torch.equal(got[k][sel], one[k].cpu()[sel]), (name, k)
        qs.append(one["q"][PLAN_MAX_GRID:].cpu())
    wrapped = torch.as_tensor(which[:n - PLAN_MAX_GRID])  # under the row of position i - cap q would have differed
    assert not torch.equal(got["q"][PLAN_MAX_GRID:], torch.stack(qs)[wrapped, torch.arange(n - PLAN_MAX_GRID)])
    env.close()


def test_both_branch_sides_in_one_launch(cuda, mid):
    """Rows with the four shape weights 0 (the eight-weight side) and shaped rows interleaved: every zero row's
    position equals plan_values / refill_values under its base, every shaped row's its set's shared-row call."""
    from runtime import kernels as K

    _, cols = mid
    sets = [X.SETS["zero4"], X.SETS["all"], _base(X.SETS["mixed"]), X.SETS["mixed"]]
    which = np.arange(N_MID) % 4
    rows = K.eval_rows(sets, device=cuda)[torch.as_tensor(which, device=cuda)].contiguous()
    got = _pv(cols, rows, 3)
    per = [K.plan_values(cols[0], cols[1], sets[0], 3, combo=cols[2]), _pv(cols, K.eval_rows(sets[1], device=cuda), 3),
           K.plan_values(cols[0], cols[1], sets[2], 3, combo=cols[2]), _pv(cols, K.eval_rows(sets[3], device=cuda), 3)]
    _same(got, _gathered(per, which, PV_KEYS), PV_KEYS, "plan values, both sides")
    assert not torch.equal(per[0]["q"], per[1]["q"]) and not torch.equal(per[2]["q"], per[3]["q"])

    board, combo = cols[0][:64].contiguous(), cols[2][:64].contiguous()
    rrows, w64 = rows[:64].contiguous(), which[:64]
    kw = dict(combo=combo, depth=3, want=RV_KEYS)
    rgot = K.refill_values_ext(board, rrows, 8, 21, **kw)
    rper = [K.refill_values(board, sets[0], 8, 21, **kw), K.refill_values_ext(board, K.eval_rows(sets[1], device=cuda), 8, 21, **kw),
            K.refill_values(board, sets[2], 8, 21, **kw), K.refill_values_ext(board, K.eval_rows(sets[3], device=cuda), 8, 21, **kw)]
    _same(rgot, _gathered(rper, w64, RV_KEYS), RV_KEYS, "refill values, both sides")
    assert not torch.equal(rper[0]["value"], rper[1]["value"])


def test_graph_replay_reads_rows_boards_and_outputs_of_the_moment(cuda, mid):
    from runtime import kernels as K

    _, (board, hand, combo) = mid
    first, _ = _dealt_rows(N_MID, cuda)
    second, _ = _dealt_rows(N_MID, cuda, shift=3)
    board2 = torch.roll(board, 1)
    eager = [(_pv((b, hand, combo), r, 2), K.refill_values_ext(b, r, 4, 9, combo=combo, depth=2, want=RV_KEYS))
             for b, r in ((board, first), (board2, second))]
    assert not torch.equal(eager[0][0]["q"], eager[1][0]["q"])
    assert not torch.equal(eager[0][1]["value"], eager[1][1]["value"])
    rows, live = first.clone(), board.clone()
    pv = K.plan_value_outputs(N_MID, cuda)
    rv = K.refill_value_outputs(N_MID, 4, cuda, want=RV_KEYS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # captured from the first call made with these buffers
        _pv((live, hand, combo), rows, 2, out=pv)
        K.refill_values_ext(live, rows, 4, 9, combo=combo, depth=2, out=rv)
    for (want_pv, want_rv), new in zip(eager, (None, (board2, second))):
        if new is not None:
            live.copy_(new[0])
            rows.copy_(new[1])
        for t in (*pv.values(), *rv.values()):
            t.fill_(-3)
        g.replay()
        torch.cuda.synchronize()
        _same(pv, want_pv, PV_KEYS, "graph replay, plan values")
        _same(rv, want_rv, RV_KEYS, "graph replay, refill values")


def test_handle_forms_equal_the_pos_forms_and_change_nothing(cuda, mid):
    from runtime import kernels as K

    env, (board, hand, combo) = mid
    rows, _ = _dealt_rows(N_MID, cuda, shift=2)
    stream = (torch.arange(N_MID, dtype=torch.int64, device=cuda) // 2).contiguous()
    before = env.state()
    _same(env.plan_values_ext(rows, 3), _pv((board, hand, combo), rows, 3), PV_KEYS, "plan values, own rows")
    shared = K.eval_rows(X.SETS["all"], device=cuda)
    _same(env.plan_values_ext(shared, 2, out=K.plan_value_outputs(N_MID, cuda, ("q", "safe"))),
          _pv((board, hand, combo), shared, 2), ("q", "safe"), "plan values, shared row")
    _same(env.refill_values_ext(rows, 4, 5, stream=stream, depth=3, want=RV_KEYS),
          K.refill_values_ext(board, rows, 4, 5, combo=combo, stream=stream, depth=3, want=RV_KEYS), RV_KEYS,
          "refill values, own rows")
    _same(env.refill_values_ext(shared, 4, 5), K.refill_values_ext(board, shared, 4, 5, combo=combo), ("value",),
          "refill values, shared row, stream = i")
    after = env.state()  # the RNG words are part of the state
    assert all(np.array_equal(before[k], after[k]) for k in before), "a handle form changed the state"


def test_no_legal_move_and_tensors_on_the_wrong_device(cuda, ref, mid):
    from _weights_each import no_action_positions
    from runtime import kernels as K
    from runtime.lib import BBNativeError

    board, hand = no_action_positions(ref)
    rows, _ = _dealt_rows(8, cuda)
    for depth in (1, 2, 3):
        got = K.plan_values_ext(board.to(cuda), hand.to(cuda), rows, depth)
        assert bool((got["q"] == R.INT64_MIN).all()) and bool((got["rest"] == -1).all())
        assert bool((got["leaves"] == 0).all()) and bool((got["safe"] == 0).all())
    full = RV.board_tensor([RV.FIXED_BOARDS[RV.FULL]] * 2, cuda)
    dead = K.refill_values_ext(full, K.eval_rows([X.SETS["all"], X.SETS["mixed"]], device=cuda), 4, 3, want=RV_KEYS)
    assert bool((dead["attempts"] == -100).all())
    assert dead["value"].cpu().tolist() == [[X.SETS["all"]["dead"]] * 4, [X.SETS["mixed"]["dead"]] * 4]

    env, (board, hand, combo) = mid
    host_rows = K.eval_rows(X.SETS["all"])
    dev_rows = host_rows.to(cuda)
    with pytest.raises(BBNativeError, match="rows must be"):
        env.plan_values_ext(host_rows, 3)
    with pytest.raises(BBNativeError, match="rows must be"):
        env.refill_values_ext(host_rows, 2, 1)
    with pytest.raises(BBNativeError, match="q must be"):
        env.plan_values_ext(dev_rows, 3, out={"q": torch.zeros((N_MID, 192), dtype=torch.int64)})
    with pytest.raises(BBNativeError, match="value must be"):
        env.refill_values_ext(dev_rows, 2, 1, out={"value": torch.zeros((N_MID, 2), dtype=torch.int64)})
    with pytest.raises(BBNativeError, match="rows must be"):
        K.plan_values_ext(board, hand, host_rows, 3, combo=combo)
    with pytest.raises(BBNativeError, match="rows must be"):
        K.plan_values_ext(board.cpu(), hand.cpu(), dev_rows, 3, combo=combo.cpu())
    with pytest.raises(BBNativeError, match="rows must be"):
        K.refill_values_ext(board, host_rows, 2, 1)
    with pytest.raises(BBNativeError, match="combo must be"):
        K.refill_values_ext(board, dev_rows, 2, 1, combo=combo.cpu())
    with pytest.raises(BBNativeError, match="stream must be"):
        K.refill_values_ext(board, dev_rows, 2, 1, stream=torch.zeros(N_MID, dtype=torch.int64))
    with pytest.raises(BBNativeError, match=rf"\[1, 12\] or \[{N_MID}, 12\]"):
        K.plan_values_ext(board, hand, K.eval_rows(X.SETS["all"], n=5, device=cuda), 3, combo=combo)


# ---------------------------------------------------------------------------------------------------------------
# refill_values_ext
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deals,depth", X.REFILL_CASES)
def test_refill_values_ext_equals_the_reference(cuda, ref, deals, depth):
    from runtime import kernels as K

    want = X.reference_refill(deals, depth)
    boards, combo, stream = X.refill_boards()
    board = RV.board_tensor(boards, cuda)
    combo_t, stream_t = torch.from_numpy(combo.copy()).to(cuda), torch.from_numpy(stream.copy()).to(cuda)
    for name, w in X.SETS.items():
        got = K.refill_values_ext(board, K.eval_rows(w, device=cuda), deals, X.REFILL_SEED, combo=combo_t,
                                  stream=stream_t, depth=depth, want=RV_KEYS)
        assert np.array_equal(RV.as_u32(got["hand"]), want["hand"]), name
        assert np.array_equal(got["attempts"].cpu().numpy(), want["attempts"]), name
        assert np.array_equal(got["value"].cpu().numpy(), want["value"][name]), (name, deals, depth)


def test_refill_values_ext_above_the_grid_cap_reads_its_boards_row(cuda, ref):
    """129 boards x 128 deals at depth 1: kRefillMaxGrid + 128 pairs, so the last board's pairs are reached by
    workgroups that stride.  Per-board rows, against the host backend."""
    from runtime import kernels as K

    n, deals = 129, 128
    assert n * deals == REFILL_MAX_GRID + 128
    env = _rolled(n, 30, 300, cuda)
    board, _, combo = _columns(env)
    env.close()
    rows, which = _dealt_rows(n, cuda, shift=1)
    stream = (torch.arange(n, dtype=torch.int64, device=cuda) % 5).contiguous()
    got = K.refill_values_ext(board, rows, deals, 13, combo=combo, stream=stream, depth=1, want=RV_KEYS)
    want = K.refill_values_ext(board.cpu(), rows.cpu(), deals, 13, combo=combo.cpu(), stream=stream.cpu(), depth=1,
                               want=RV_KEYS)
    _same(got, want, RV_KEYS, "above the grid cap")
    other = K.refill_values_ext(board.cpu()[-1:].contiguous(), rows.cpu()[-2:-1].contiguous(), deals, 13,
                                combo=combo.cpu()[-1:].contiguous(), stream=stream.cpu()[-1:].contiguous(), depth=1)
    assert not torch.equal(other["value"][0], want["value"][-1])  # the neighbouring row would have shown


# ---------------------------------------------------------------------------------------------------------------
# the agent
# ---------------------------------------------------------------------------------------------------------------
def test_two_hand_shape_agent_plays_the_host_backends_moves(cuda, ref):
    from agents.greedy import HandPlanAgent, TwoHandShapeAgent
    from runtime.device_env import DeviceEnvBatch

    played = {}
    for dev in (cuda, CPU):
        agent = TwoHandShapeAgent(X.SETS["all"], depth=3, candidates=4, deals=4, seed=5, device=dev)
        plain_agent = HandPlanAgent(X.SETS["all"], depth=3, device=dev)
        env = DeviceEnvBatch(4, [900 + i for i in range(4)], autoreset=False, device=dev)
        env.reset()
        out = torch.zeros(4, dtype=torch.int32, device=dev)
        plain = torch.zeros_like(out)
        moves, differs = [], 0
        for _ in range(30):
            plain_agent.act_env(env, plain)
            agent.act_env(env, out)
            differs += int((plain != out).sum())
            moves.append(out.cpu().clone())
            env.step(out)
        played[dev.type] = (torch.stack(moves), env.state()["score"].copy(), differs)
        env.close()
    assert torch.equal(played["cuda"][0], played["cpu"][0]) and np.array_equal(played["cuda"][1], played["cpu"][1])
    assert played["cuda"][2] >= 1  # the look past the refill changes a move
