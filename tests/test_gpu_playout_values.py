"""bb_playout_values(_pos) on the GPU against tests/_playout_ref.py: the oracle's recorded answer on the tiny case
(tests/golden/playout_tiny.json, held to the oracle itself by tests/test_playout_values_host.py), the composition of the
existing entry points on crowded census boards, and the host backend at the grid cap.  Integer-exact, every output.
What a case is for is asserted from the reference's answers."""
import numpy as np
import pytest
import torch

import _playout_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def golden():
    return PR.tiny_golden()


@pytest.fixture(scope="module")
def crowded(cuda, lib):
    """The 36 census boards (crowded, open, full, checker) with combos, stream ids shared in pairs and rows of all
    kinds in turn: shaped, zero-shape, anti-play, score-weighing."""
    import _census_ref as CR

    bs = CR.boards()
    n = len(bs)
    kinds = PR.rows_of([PR.SHAPED, PR.PLAIN, PR.ANTI, PR.SCORED])
    return {"np": bs, "n": n, "board": PR.board_tensor(bs, cuda),
            "combo": (torch.arange(n) % 5).to(torch.int32).to(cuda),
            "stream": (torch.arange(n) // 2 + 5).to(torch.int64).to(cuda),
            "rows": torch.stack([kinds[i % 4] for i in range(n)]).contiguous().to(cuda)}


def test_the_smallest_call_against_the_oracle(cuda, lib, golden):
    """n = 1, one playout, one hand: board 3 of the tiny case alone keeps its stream id and so its first deal."""
    board, rows, combo, stream = PR.tiny_tensors(cuda)
    got = PR.call(board[3:4].contiguous(), rows[3:4].contiguous(), 3, 1, 1, PR.TINY_SEED,
                  combo=combo[3:4].contiguous(), stream=stream[3:4].contiguous())
    PR.assert_equal(got, {k: v[3:4, :1] for k, v in golden[1].items()}, "n=1")


@pytest.mark.parametrize("hands", [1, 2, 3])
def test_five_boards_eight_playouts_against_the_oracle(cuda, lib, golden, hands):
    """Shaped and unshaped rows in one launch (w_stride 1), shared stream ids, combos carried in; at hands == 3 the
    launch holds all the endings: survived, dead leaf (at hand 1 and at hand 2), no legal first move."""
    board, rows, combo, stream = PR.tiny_tensors(cuda)
    got = PR.call(board, rows, 3, PR.TINY_PLAYOUTS, hands, PR.TINY_SEED, combo=combo, stream=stream)
    PR.assert_equal(got, golden[hands], f"hands {hands}")
    survived, dead, cut, none = PR.endings(golden[hands])
    assert survived >= 8 and dead >= 3 and none >= 8
    if hands == 3:
        assert ((golden[3]["status"] & PR.PP.DEAD != 0) & (golden[3]["hands"] == 2)).any()
        assert {1, 2, 3} <= set(golden[3]["hands"].reshape(-1).tolist())


@pytest.mark.parametrize("depth,hands", [(3, 3), (2, 2), (1, 1)])
def test_the_census_boards_against_the_composed_entry_points(cuda, lib, crowded, depth, hands):
    c = crowded
    want = PR.composed(c["board"], c["rows"], depth, 4, hands, 5, combo=c["combo"], stream=c["stream"])
    got = PR.call(c["board"], c["rows"], depth, 4, hands, 5, combo=c["combo"], stream=c["stream"])
    PR.assert_equal(got, want, f"depth {depth} hands {hands}")
    survived, dead, cut, none = PR.endings(want)
    if depth == 3:  # all three endings in one launch
        assert survived > 100 and dead >= 2 and none >= 4
    else:
        assert survived == 0 and cut > 100
    one = c["rows"][:1].contiguous()  # w_stride 0 against the same row repeated
    a = PR.call(c["board"], one, depth, 4, hands, 5, combo=c["combo"], stream=c["stream"])
    b = PR.call(c["board"], one.expand(c["n"], 12).contiguous(), depth, 4, hands, 5, combo=c["combo"], stream=c["stream"])
    PR.assert_equal(a, b, "shared row")


def test_the_carried_combo_and_the_seed_wrap(cuda, lib, crowded):
    c = crowded
    rows = PR.rows_of(PR.SCORED, cuda)  # a row that weighs the score: the combo shows there alone
    want = PR.composed(c["board"], rows, 3, 4, 3, 5)
    wrong = PR.composed(c["board"], rows, 3, 4, 3, 5, carry_combo=False)
    got = PR.call(c["board"], rows, 3, 4, 3, 5)
    PR.assert_equal(got, want, "carried")
    assert (want["value"] != wrong["value"]).any() and (want["score"] != wrong["score"]).any()
    top = 2 ** 64 - 1  # the second hand's key wraps to 0, as ``composed`` keys it
    few = c["board"][:8].contiguous()
    got = PR.call(few, rows, 3, 4, 2, top)
    PR.assert_equal(got, PR.composed(few, rows, 3, 4, 2, top), "wrap")
    assert bool((got["hands"] == 2).any())


def test_streams_and_the_two_forms(cuda, lib, crowded):
    from runtime.device_env import DeviceEnvBatch

    c, n = crowded, crowded["n"]
    twice = torch.cat([c["board"], c["board"]]).contiguous()
    rows2 = torch.cat([c["rows"], c["rows"]]).contiguous()
    combo2 = torch.cat([c["combo"], c["combo"]]).contiguous()
    stream = torch.cat([torch.arange(n), torch.arange(n)]).to(torch.int64).to(cuda)
    got = PR.call(twice, rows2, 3, 3, 2, 8, combo=combo2, stream=stream)
    for key in PR.OUTPUTS:  # equal boards, rows, combos and stream ids: equal rows
        assert torch.equal(got[key][:n], got[key][n:]), key
    plain = PR.call(twice, rows2, 3, 3, 2, 8, combo=combo2)  # NULL = i: the second half draws from other streams
    ident = PR.call(twice, rows2, 3, 3, 2, 8, combo=combo2, stream=torch.arange(2 * n, dtype=torch.int64, device=cuda))
    for key in PR.OUTPUTS:
        assert torch.equal(plain[key], ident[key]), key
    assert not torch.equal(plain["hand"][:n], plain["hand"][n:])
    # the handle form reads the live columns and changes nothing, the RNG included
    env = DeviceEnvBatch(8, list(range(40, 48)), autoreset=False, device=cuda)
    env.reset()
    act = torch.zeros(8, dtype=torch.int32, device=cuda)
    for _ in range(7):
        env.plan_actions(act, PR.R.DEFAULT_WEIGHTS, 1)
        env.step(act)
    before = env.state()
    rows = c["rows"][:8].contiguous()
    live = env.playout_values(rows, 3, 2, 21, want=PR.OUTPUTS)
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    same = PR.call(PR.board_tensor(before["board"], cuda), rows, 3, 3, 2, 21,
                   combo=torch.from_numpy(before["combo"].astype(np.int32)).to(cuda))
    PR.assert_equal(live, same, "handle")
    env.step(act)  # the piece streams go on as if nothing had been asked
    env.close()


def test_the_grid_cap_against_the_host_backend(cuda, lib, host, crowded):
    """129 boards x 128 playouts = 16,512 pairs, above the 16,384 of the grid: the workgroups of pairs 0..127 take a
    second pair, (board 128, playout j) behind (board 0, playout j) -- the full board behind a dense one, so one hand
    searched behind two, and no legal first move behind a playout that survived."""
    bs = crowded["np"]
    n, m = 129, 128
    pool = np.array([5, 2, 6, 7, 3, 8, 9, 10, 11, 12, 13, 14])  # dense boards, the checker and the checker with a free row
    rep = pool[np.arange(n) % len(pool)]
    rep[128] = 1  # the full board
    boards = bs[rep]
    kinds = PR.rows_of([PR.SHAPED, PR.PLAIN, PR.ANTI, PR.SCORED])
    rows = torch.stack([kinds[i % 4] for i in range(n)]).contiguous()
    stream = torch.from_numpy((np.arange(n) % 50).astype(np.int64))
    want = PR.call(PR.board_tensor(boards), rows, 3, m, 2, 6, stream=stream)
    got = PR.call(PR.board_tensor(boards, cuda), rows.to(cuda), 3, m, 2, 6, stream=stream.to(cuda))
    PR.assert_equal(got, want, "grid cap")
    assert n * m > 1 << 14 and bool((want["hands"][0] == 2).all()) and bool((want["hands"][128] == 1).all())
    survived, dead, cut, none = PR.endings(want)
    assert survived > 10000 and dead > 100 and none > m and cut == 0


def test_guard_words_each_output_alone_and_wrong_devices(cuda, lib, crowded):
    c = crowded
    n, m = 12, 5
    board, rows = c["board"][:n].contiguous(), c["rows"][:n].contiguous()
    combo, stream = c["combo"][:n].contiguous(), c["stream"][:n].contiguous()
    want = PR.call(board, rows, 3, m, 2, 13, combo=combo, stream=stream)
    bufs = {key: PR.guarded(n, m, cuda, key) for key in PR.OUTPUTS}
    got = PR.call(board, rows, 3, m, 2, 13, combo=combo, stream=stream, out={key: v for key, (_, v) in bufs.items()})
    torch.cuda.synchronize()
    PR.assert_equal(got, want, "guarded")
    assert all(PR.guards_intact(b) for b, _ in bufs.values())
    for key in PR.OUTPUTS:  # each output alone
        buf, view = PR.guarded(n, m, cuda, key)
        PR.call(board, rows, 3, m, 2, 13, combo=combo, stream=stream, out={key: view})
        torch.cuda.synchronize()
        assert torch.equal(view, want[key]) and PR.guards_intact(buf), key
    with pytest.raises(Exception, match="on cuda"):
        PR.call(board, rows.cpu(), 3, m, 2, 13)
    with pytest.raises(Exception, match="on cuda"):
        PR.call(board, rows, 3, m, 2, 13, stream=stream.cpu())
    with pytest.raises(Exception, match="on cuda"):
        PR.call(board, rows, 3, m, 2, 13, combo=combo.cpu())
    with pytest.raises(Exception, match="on cuda"):
        PR.call(board, rows, 3, m, 2, 13, out={"value": torch.zeros((n, m), dtype=torch.int64)})


def test_graph_capture_from_the_first_call(cuda, lib, crowded):
    """Captured on the very first call with these sizes, replayed after boards, rows and outputs were rewritten; the
    seed is an argument by value, so the replay repeats the deals of the capture."""
    from runtime import kernels as K

    c = crowded
    n, m = 10, 6
    src_board, src_rows = c["board"][2:2 + n].clone(), c["rows"][2:2 + n].clone()
    src_combo = c["combo"][2:2 + n].clone()
    board, rows, combo = torch.zeros_like(src_board), torch.zeros_like(src_rows), torch.zeros_like(src_combo)
    out = K.playout_outputs(n, m, cuda, PR.OUTPUTS)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            PR.call(board, rows, 3, m, 3, 99, combo=combo, out=out)
    board.copy_(src_board)
    rows.copy_(src_rows)
    combo.copy_(src_combo)
    for v in out.values():
        v.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    want = PR.composed(src_board, src_rows, 3, m, 3, 99, combo=src_combo)
    PR.assert_equal(out, want, "replay")
    assert PR.endings(want)[0] > 10


def test_the_agent_plays_the_hosts_moves(cuda, lib, host):
    """PlayoutPlanAgent: 8 envs x 12 moves on the GPU equal to the host backend's."""
    import _plan2_ref as P2
    from agents import PlayoutPlanAgent

    seeds = list(range(70, 78))
    logs = [P2.play(PlayoutPlanAgent(PR.SHAPED, candidates=4, deals=4, hands=2, seed=3, device=dev), seeds, 12, dev)
            for dev in ("cpu", cuda)]
    assert logs[0] == logs[1]
