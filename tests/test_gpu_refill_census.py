"""The refill census on the MI355X (bb_refill_census / bb_refill_census_pos of libbbvec.so, csrc/bb_census.hip),
against tests/_census_ref.py's oracle census, which calls neither:

* n = 1 (empty / full / checkerboard in turn), n = 5 and the whole reference set, stateless and handle form, count
  alone, words alone and both;
* more boards than the grid cap, dealt round-robin from the reference set so that the boards a workgroup strides
  over differ;
* a second reference on the GPU: bb_safe_mask_pos over the 9,139 replicated hands of four boards;
* a graph captured once and replayed on boards rewritten in place;
* guard words around both outputs, and tensors on the wrong side.
"""
import numpy as np
import pytest
import torch

import _census_ref as CR

pytestmark = pytest.mark.gpu

CENSUS_MAX_GRID = 1 << 11  # kCensusMaxGrid of csrc/bb_census.hip
FILL = -7


def _check(out, idx, what):
    ref = CR.reference()
    if "count" in out:
        assert out["count"].cpu().tolist() == ref["count"][idx].tolist(), what
    if "solvable" in out:
        bad = np.argwhere(CR.as_u64(out["solvable"]) != ref["solvable"][idx])
        assert bad.size == 0, (what, bad[:4].tolist())


@pytest.mark.parametrize("want", [("count",), ("solvable",), ("count", "solvable")], ids=["count", "words", "both"])
@pytest.mark.parametrize("which", ["empty", "full", "checker", "first5", "all"])
def test_pos_form_equals_the_oracle(cuda, which, want):
    from runtime import kernels as K

    ref = CR.reference()
    names = list(CR.NAMED)
    idx = {"first5": np.arange(5), "all": np.arange(len(ref["board"]))}.get(which)
    idx = np.array([names.index(which)]) if idx is None else idx
    out = K.refill_census(CR.board_tensor(ref["board"][idx], cuda), want=want)
    assert set(out) == set(want)
    _check(out, idx, which)


@pytest.mark.parametrize("want", [("count",), ("solvable",), ("count", "solvable")], ids=["count", "words", "both"])
def test_handle_form_equals_the_oracle_and_changes_nothing(cuda, want):
    from runtime.device_env import DeviceEnvBatch

    ref = CR.reference()
    n = len(ref["board"])
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    env.set_state(board=ref["board"])
    before = env.state()
    bufs = {"count": torch.full((n,), FILL, dtype=torch.int32, device=cuda),
            "solvable": torch.full((n, 37, 37), FILL, dtype=torch.int64, device=cuda)}
    out = env.refill_census(**{k: bufs[k] for k in want})
    assert set(out) == set(want)
    _check(out, np.arange(n), "handle")
    for k in set(bufs) - set(want):
        assert (bufs[k] == FILL).all(), f"{k} was not asked for"
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


def test_more_boards_than_workgroups(cuda):
    """n = the grid cap + 3, board i = reference board i mod 36: 2,048 is no multiple of 36, so the boards i and
    i + cap that one workgroup takes differ (and so do clogged and open neighbours)."""
    from runtime import kernels as K

    ref = CR.reference()
    m = len(ref["board"])
    n = CENSUS_MAX_GRID + 3
    idx = np.arange(n) % m
    assert CENSUS_MAX_GRID % m != 0 and (ref["count"][idx[:3]] != ref["count"][idx[CENSUS_MAX_GRID:]]).any()
    out = K.refill_census(CR.board_tensor(ref["board"][idx], cuda))
    got = out["count"].cpu().numpy()
    bad = np.nonzero(got != ref["count"][idx])[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist())


def test_safe_mask_over_the_replicated_hands_gives_the_same_counts(cuda):
    """The chain the census replaces: bb_safe_mask_pos mode 0 on 9,139 (board, hand) replicas per board, a hand
    counted with its multiplicity where any first move is safe."""
    from runtime import kernels as K

    ref = CR.reference()
    idx = np.array([2, 3, 6, 20])  # the two checkerboards, a crowded and a sparse board
    boards = CR.board_tensor(np.repeat(ref["board"][idx], len(CR.MULTISETS)), cuda)
    hands = torch.from_numpy(np.tile(CR.HAND_WORDS, len(idx)).view(np.int32).copy()).to(cuda)
    safe = K.safe_mask(boards, hands, K.SAFE_WORDS)
    ok = (safe != 0).any(dim=1).reshape(len(idx), -1).cpu().numpy()
    chain = (ok * CR.MULTIPLICITY).sum(axis=1)
    got = K.refill_census(CR.board_tensor(ref["board"][idx], cuda))["count"].cpu().numpy()
    assert chain.tolist() == got.tolist() == ref["count"][idx].tolist()


def test_graph_capture_and_replay_on_rewritten_boards(cuda):
    from runtime import kernels as K

    ref = CR.reference()
    n = 6
    sets = [np.arange(0, 6), np.arange(6, 12), np.arange(20, 26)]
    board = CR.board_tensor(ref["board"][sets[0]], cuda)
    out = {"count": torch.full((n,), FILL, dtype=torch.int32, device=cuda),
           "solvable": torch.full((n, 37, 37), FILL, dtype=torch.int64, device=cuda)}
    K.refill_census(board, out=out)  # the piece table is built before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.refill_census(board, out=out)
    for idx in sets:
        board.copy_(CR.board_tensor(ref["board"][idx], cuda))
        out["count"].fill_(FILL)
        out["solvable"].fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        _check(out, idx, f"graph replay on boards {idx[0]}..")


def test_nothing_written_beyond_the_outputs(cuda):
    from runtime import kernels as K

    ref = CR.reference()
    n = len(ref["board"])
    board = CR.board_tensor(ref["board"], cuda)
    count = torch.full((n + 16,), FILL, dtype=torch.int32, device=cuda)
    words = torch.full((n * 1369 + 16,), FILL, dtype=torch.int64, device=cuda)
    out = {"count": count[8:8 + n], "solvable": words[8:8 + n * 1369].view(n, 37, 37)}
    K.refill_census(board, out=out)
    _check(out, np.arange(n), "guarded")
    assert (count[:8] == FILL).all() and (count[8 + n:] == FILL).all()
    assert (words[:8] == FILL).all() and (words[8 + n * 1369:] == FILL).all()
    words.fill_(FILL)
    K.refill_census(board, out={"count": out["count"]})
    assert (words == FILL).all()  # solvable NULL: not a word of it is written


def test_tensors_on_the_wrong_side_are_refused(cuda):
    from runtime import kernels as K
    from runtime import lib as L

    b = CR.board_tensor(CR.reference()["board"][:4])
    with pytest.raises(L.BBNativeError, match="count must be a contiguous"):
        K.refill_census(b.to(cuda), out={"count": torch.zeros(4, dtype=torch.int32)})
    with pytest.raises(L.BBNativeError, match="solvable must be a contiguous"):
        K.refill_census(b, out={"solvable": torch.zeros((4, 37, 37), dtype=torch.int64, device=cuda)})
