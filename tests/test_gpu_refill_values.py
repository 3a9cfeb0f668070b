"""Dealt next-hand values on the MI355X (bb_refill_values / bb_refill_values_pos of libbbvec.so, refill_values_kernel in
csrc/bb_lookahead.hip):

* HIP = tests/_refill_values_ref.py on the fixed case: n = 1 (each board in turn) and n = 5, 1 and 8 deals, depth 1-3,
  stateless and handle form, each output alone between guard words;
* HIP = the host backend on the 36 boards of tests/_census_ref.py dealt round-robin over more (board, deal) pairs
  than the grid cap, so that the pairs one workgroup strides over differ;
* the dealt hands fed back through bb_plan_actions_pos give the values;
* a graph captured once and replayed after the boards and combos are rewritten in place;
* tensors on the wrong side are refused.
"""
import numpy as np
import pytest
import torch

import _census_ref as CR
import _refill_values_ref as RV

pytestmark = pytest.mark.gpu

WANT = ("hand", "value", "attempts")
FILL = -7
SCORED = {"lines": 10, "score": 1, "holes": -3, "filled": -1, "dead": -5000}


def _check_fixed(out, ref, rows, deals, what):
    for k in out:
        got = out[k].cpu().numpy()
        got = got.view(np.uint32) if k == "hand" else got
        assert got.tolist() == ref[k][rows][:, :deals].tolist(), (what, k)


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("deals", [1, 8])
def test_pos_form_equals_the_reference_on_the_fixed_case(cuda, depth, deals):
    """Deal j does not depend on the number of deals, so the first column of the 8-deal reference is the 1-deal one."""
    from runtime import kernels as K

    ref = RV.fixed(depth)
    for rows in [np.arange(5)] + [np.array([i]) for i in range(5)]:
        if len(rows) == 1 and rows[0] != 0:
            # stream = i: board i alone sits at index 0, so its reference stream id is passed explicitly
            stream = torch.tensor(rows, dtype=torch.int64, device=cuda)
        else:
            stream = None
        out = K.refill_values(RV.board_tensor(RV.FIXED_BOARDS[rows], cuda), RV.WEIGHTS, deals, RV.FIXED_SEED,
                              stream=stream, depth=depth, want=WANT)
        assert set(out) == set(WANT) and all(t.shape == (len(rows), deals) for t in out.values())
        _check_fixed(out, ref, rows, deals, rows.tolist())


@pytest.mark.parametrize("depth", [1, 3])
def test_handle_form_equals_the_reference_and_changes_nothing(cuda, depth):
    from runtime.device_env import DeviceEnvBatch

    ref = RV.fixed(depth)
    env = DeviceEnvBatch(5, [1, 2, 3, 4, 5], autoreset=False, device=cuda)
    env.reset()
    env.set_state(board=RV.FIXED_BOARDS, combo=np.zeros(5, np.int32))
    before = env.state()
    out = env.refill_values(RV.WEIGHTS, RV.FIXED_DEALS, RV.FIXED_SEED, depth=depth, want=WANT)
    _check_fixed(out, ref, np.arange(5), RV.FIXED_DEALS, "handle")
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


@pytest.mark.parametrize("wanted", [("hand",), ("value",), ("attempts",), WANT], ids=["hand", "value", "attempts", "all"])
def test_each_output_alone_between_guard_words(cuda, wanted):
    from runtime import kernels as K

    ref = RV.fixed(2)
    n, m = 5, RV.FIXED_DEALS
    bufs = {k: torch.full((n * m + 16,), FILL, dtype=dt, device=cuda) for k, dt in K.REFILL_VALUE_OUTPUTS.items()}
    out = {k: bufs[k][8:8 + n * m].view(n, m) for k in wanted}
    K.refill_values(RV.board_tensor(RV.FIXED_BOARDS, cuda), RV.WEIGHTS, m, RV.FIXED_SEED, depth=2, out=out)
    _check_fixed(out, ref, np.arange(n), m, wanted)
    for k, v in bufs.items():
        assert (v[:8] == FILL).all() and (v[8 + n * m:] == FILL).all(), k
        if k not in wanted:
            assert (v == FILL).all(), f"{k} was not asked for"


def test_more_pairs_than_workgroups_equal_the_host_backend(cuda):
    """(board, deal) pairs = the grid cap + 3 and a few more, board i = census board i mod 36, three deals each, combos
    0..7 and a stream id shared by neighbours: the pair a workgroup takes after its first differs from it in board and
    deal.  Depth 1 keeps the host's side quick; the dealer's search does not depend on the depth."""
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    bs = CR.boards()
    deals = 3
    n = (K.REFILL_MAX_GRID + 3 + deals - 1) // deals
    idx = np.arange(n) % len(bs)
    pair_board = np.repeat(bs[idx], deals)
    assert n * deals >= K.REFILL_MAX_GRID + 3 and K.REFILL_MAX_GRID % deals != 0
    assert (pair_board[:3] != pair_board[K.REFILL_MAX_GRID:K.REFILL_MAX_GRID + 3]).all()
    board = CR.board_tensor(bs[idx])
    combo = torch.from_numpy((np.arange(n) % 8).astype(np.int32))
    stream = torch.from_numpy((np.arange(n) // 2).astype(np.int64))
    want = K.refill_values(board, SCORED, deals, 5, combo=combo, stream=stream, depth=1, want=WANT)
    got = K.refill_values(board.to(cuda), SCORED, deals, 5, combo=combo.to(cuda), stream=stream.to(cuda), depth=1,
                          want=WANT)
    for k in WANT:
        bad = torch.nonzero(got[k].cpu() != want[k])[:4]
        assert bad.numel() == 0, (k, bad.tolist())
    at = want["attempts"]
    assert (at == 1).any() and ((at > 1) & (at < 100)).any() and (at == -100).any()


@pytest.mark.parametrize("depth", [2, 3])
def test_hands_fed_back_through_plan_actions_give_the_values(cuda, depth):
    from runtime import kernels as K

    bs = CR.boards()
    n, deals = len(bs), 4
    board = CR.board_tensor(bs, cuda)
    combo = (torch.arange(n, dtype=torch.int32, device=cuda) % 6).contiguous()
    out = K.refill_values(board, SCORED, deals, 123, combo=combo, depth=depth, want=("hand", "value"))
    plan = K.plan_actions(board.repeat_interleave(deals), out["hand"].reshape(-1).contiguous(), SCORED, depth,
                          combo=combo.repeat_interleave(deals))
    want = torch.where(plan["value"] == torch.iinfo(torch.int64).min, SCORED["dead"], plan["value"])
    assert torch.equal(out["value"].reshape(-1), want)
    assert (plan["value"] == torch.iinfo(torch.int64).min).any()  # the full board: no legal first move


def test_graph_capture_and_replay_on_rewritten_boards_and_combos(cuda):
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    bs = CR.boards()
    n, deals = 6, 4
    sets = [np.arange(0, 6), np.arange(6, 12), np.arange(20, 26)]
    board = CR.board_tensor(bs[sets[0]], cuda)
    combo = torch.zeros(n, dtype=torch.int32, device=cuda)
    out = {k: torch.full((n, deals), FILL, dtype=dt, device=cuda) for k, dt in K.REFILL_VALUE_OUTPUTS.items()}
    K.refill_values(board, SCORED, deals, 31, combo=combo, depth=3, out=out)  # the piece table is built before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.refill_values(board, SCORED, deals, 31, combo=combo, depth=3, out=out)
    for r, idx in enumerate(sets):
        cb = torch.full((n,), 2 * r, dtype=torch.int32)
        board.copy_(CR.board_tensor(bs[idx], cuda))
        combo.copy_(cb)
        for t in out.values():
            t.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        want = K.refill_values(CR.board_tensor(bs[idx]), SCORED, deals, 31, combo=cb, depth=3, want=WANT)
        for k in WANT:
            assert torch.equal(out[k].cpu(), want[k]), (k, r)


def test_tensors_on_the_wrong_side_are_refused(cuda):
    from runtime import kernels as K
    from runtime import lib as L

    b = RV.board_tensor(RV.FIXED_BOARDS)
    with pytest.raises(L.BBNativeError, match="value must be a contiguous"):
        K.refill_values(b.to(cuda), RV.WEIGHTS, 2, 1, out={"value": torch.zeros((5, 2), dtype=torch.int64)})
    with pytest.raises(L.BBNativeError, match="hand must be a contiguous"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, out={"hand": torch.zeros((5, 2), dtype=torch.int32, device=cuda)})
    with pytest.raises(L.BBNativeError, match="combo must be a contiguous"):
        K.refill_values(b.to(cuda), RV.WEIGHTS, 2, 1, combo=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(L.BBNativeError, match="stream must be a contiguous"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, stream=torch.zeros(5, dtype=torch.int64, device=cuda))
