"""bb_plan2_values(_pos) on the GPU against tests/_plan2_ref.py: the oracle restatement on a handful of positions,
the composition of the existing entry points (``composed``) on the whole position set, and the host backend at the
grid caps.  Integer-exact, every output.  What a case is for is asserted from the reference's answers."""
import numpy as np
import pytest
import torch

import _plan2_ref as P2

pytestmark = pytest.mark.gpu
INT64_MIN = P2.INT64_MIN


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def pos(cuda, lib):
    board, hand, combo, names = P2.positions()
    tb, th, tc = P2.to_tensors(board, hand, combo, cuda)
    return {"np": (board, hand, combo), "t": (tb, th, tc), "names": names, "n": len(board),
            "rows": P2.mixed_rows(len(board), cuda)}


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_smallest_calls_against_the_oracle(cuda, lib, pos, depth):
    from runtime import kernels as K

    board, hand, combo = pos["np"]
    # one position, one candidate, one deal: a mid-game position of the played set
    sel = [20]
    want = P2.oracle(board[sel], hand[sel], combo[sel], P2.SHAPED, depth, 1, 1, 5)
    got = P2.call(*P2.to_tensors(board, hand, combo, cuda, sel), K.eval_rows(P2.SHAPED, device=cuda), depth, 1, 1, 5)
    P2.assert_equal(got, want, "n=1")
    # five positions, three candidates, two deals, a row each and shared stream ids
    sel = [3, 31, 47, pos["names"]["one_slot_left"], pos["names"]["combo5_row_short"]]
    ws = [P2.SHAPED, P2.PLAIN, P2.SHAPED, P2.PLAIN, {**P2.SHAPED, "score": 3}]  # the combo shows in the score alone
    stream = [4, 4, 9, 1, 0]
    rows = torch.cat([K.eval_rows(w) for w in ws]).to(cuda)
    t5 = P2.to_tensors(board, hand, combo, cuda, sel)
    ts = torch.tensor(stream, dtype=torch.int64, device=cuda)
    if depth < 3:
        want = P2.oracle(board[sel], hand[sel], combo[sel], ws, depth, 3, 2, 77, stream=stream)
    else:  # thirty dealt hands searched three plies deep take the oracle a minute: the composed entry points instead
        want = P2.as_numpy(P2.composed(*t5, rows, depth, 3, 2, 77, stream=ts))
    got = P2.call(*t5, rows, depth, 3, 2, 77, stream=ts)
    P2.assert_equal(got, want, "n=5")
    refill, _, _ = P2.leaf_kinds(want)
    assert refill >= 6  # the two crafted positions deal behind every candidate
    # the carried combo: the candidates of combo5_row_short (root combo 5) are dealt under their leaves' combos -- 6 behind
    # the clearing move, 0 behind the others -- and dealing under the root's combo would give other values
    wrong = P2.as_numpy(P2.composed(*t5, rows, depth, 3, 2, 77, stream=ts, deal_combo="root"))
    assert want["cand"][4][0] >= 0 and (wrong["value"][4] != want["value"][4]).any()
    assert (wrong["value"][:3] == want["value"][:3]).all()  # the whole hands of the played games: no deal at depth < 3, or the same combo


@pytest.mark.parametrize("depth,k,deals", [(1, 5, 3), (2, 8, 3), (3, 3, 2)])
def test_the_position_set_against_the_composed_entry_points(cuda, lib, pos, depth, k, deals):
    """Rows of all kinds in one launch (shaped, zero-shape, all zeros), stream ids shared in pairs."""
    n = pos["n"]
    stream = (torch.arange(n, device=cuda) // 2).to(torch.int64)
    want = P2.composed(*pos["t"], pos["rows"], depth, k, deals, 3, stream=stream)
    got = P2.call(*pos["t"], pos["rows"], depth, k, deals, 3, stream=stream)
    P2.assert_equal(got, want, f"depth {depth}")
    refill, dead, cut = P2.leaf_kinds(want)
    assert refill > 20 and dead > 10 and (cut > 20 or depth == 3)  # all the leaf kinds in one launch
    w = P2.as_numpy(want)
    present, is_refill = w["status"] >= 0, (w["status"] >= 0) & ((w["status"] & 8) != 0)
    assert not w["value"][~is_refill].any() and (~present).any()
    names = pos["names"]
    for name in ("game_over_bit", "all_used", "full_but_one"):  # no legal action
        i = names[name]
        assert int(got["action"][i]) == 0 and bool((got["q2"][i] == INT64_MIN).all()) and bool((got["cand"][i] == -1).all())
    if depth == 2:  # a whole hand is cut short by depth 2; a hand with one slot left refills
        assert (w["status"][names["whole_hand"]] & 12 == 0).all() and (w["status"][names["one_slot_left"]] & 8).all()


def test_ties_go_to_the_lower_action_not_the_lower_rank(cuda, lib, pos):
    from runtime import kernels as K

    n = pos["n"]
    zero = K.eval_rows(P2.ZERO12, device=cuda)
    got = P2.call(*pos["t"], zero, 2, 6, 2, 1)
    legal = P2.composed(*pos["t"], zero, 2, 192, 1, 1)["cand"]
    for i in range(n):  # every q and every Q2 is 0: the K lowest legal actions, and the lowest of them
        want = legal[i][:6]
        assert torch.equal(got["cand"][i], want)
        assert int(got["action"][i]) == (int(want[0]) if int(want[0]) >= 0 else 0)
    # rank order differing from action order (col_short of tests/_plan2_ref.py): action 184 clears the column and ranks
    # first; action 129 keeps it, and the dealt hand finishes it, so Q2 ties and the lower action wins over the rank
    rows = K.eval_rows({**P2.ZERO12, "lines": 1}, device=cuda)
    want = P2.as_numpy(P2.composed(*pos["t"], rows, 1, 4, 1, TIE_SEED))
    got = P2.call(*pos["t"], rows, 1, 4, 1, TIE_SEED)
    P2.assert_equal(got, want, "rank order")
    i = pos["names"]["col_short"]
    assert want["cand"][i].tolist() == [184, 129, 130, 131] and want["q2"][i, 184] == want["q2"][i, 129] == 1
    assert want["action"][i] == 129 and int(got["action"][i]) == 129


TIE_SEED = 2  # a seed under which stream `col_short` is dealt a piece that finishes the column (asserted above)


def test_more_candidates_than_legal_actions(cuda, lib, pos):
    from runtime import kernels as K

    rows = K.eval_rows(P2.SHAPED, device=cuda)
    want = P2.composed(*pos["t"], rows, 1, 192, 1, 4)
    got = P2.call(*pos["t"], rows, 1, 192, 1, 4)
    P2.assert_equal(got, want, "K=192")
    present = (want["cand"] >= 0).sum(dim=1)
    assert int(present[pos["names"]["empty_singles"]]) == 192  # more than one candidate a lane in the pick
    assert int((present > 0).sum()) > 100 and int(((present > 0) & (present < 20)).sum()) >= 5  # -1 tails


def test_streams_rows_and_the_two_forms(cuda, lib, pos):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    tb, th, tc = pos["t"]
    n = pos["n"]
    twice = [torch.cat([t, t]).contiguous() for t in (tb, th, tc)]
    rows2 = torch.cat([pos["rows"], pos["rows"]]).contiguous()
    stream = torch.cat([torch.arange(n), torch.arange(n)]).to(torch.int64).to(cuda)
    got = P2.call(*twice, rows2, 2, 4, 3, 8, stream=stream)
    for key in P2.OUTPUTS:  # equal boards, hands, rows and stream ids: equal outputs
        assert torch.equal(got[key][:n], got[key][n:]), key
    plain = P2.call(*twice, rows2, 2, 4, 3, 8)  # NULL = i: the second half draws from other streams
    ident = P2.call(*twice, rows2, 2, 4, 3, 8, stream=torch.arange(2 * n, dtype=torch.int64, device=cuda))
    for key in P2.OUTPUTS:
        assert torch.equal(plain[key], ident[key]), key
    assert not torch.equal(plain["value"][:n], plain["value"][n:])
    # w_stride 0 against the same row repeated; the dealt values use the root's row
    one = K.eval_rows(P2.SHAPED, device=cuda)
    a = P2.call(tb, th, tc, one, 2, 4, 3, 8)
    b = P2.call(tb, th, tc, one.expand(n, 12).contiguous(), 2, 4, 3, 8)
    c = P2.call(tb, th, tc, K.eval_rows(P2.PLAIN, device=cuda), 2, 4, 3, 8)
    for key in P2.OUTPUTS:
        assert torch.equal(a[key], b[key]), key
    assert not torch.equal(a["value"], c["value"])
    # the handle form reads the live columns and changes nothing, the RNG included
    env = DeviceEnvBatch(8, list(range(40, 48)), autoreset=False, device=cuda)
    env.reset()
    act = torch.zeros(8, dtype=torch.int32, device=cuda)
    for _ in range(7):
        env.plan_actions(act, P2.R.DEFAULT_WEIGHTS, 1)
        env.step(act)
    before = env.state()
    rows = P2.mixed_rows(8, cuda)
    live = env.plan2_values(rows, 4, 3, 21, want=P2.OUTPUTS)
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    eb, eh, ec = P2.to_tensors(before["board"], before["hand"], before["combo"], cuda)
    same = P2.call(eb, eh, ec, rows, 3, 4, 3, 21)
    for key in P2.OUTPUTS:
        assert torch.equal(live[key], same[key]), key
    env.close()


def test_the_grid_caps_against_the_host_backend(cuda, lib, host, pos):
    from runtime import kernels as K

    board, hand, combo = pos["np"]
    # 17 roots x 8 candidates x 128 deals = 17,408 triples, above the 16,384 of the deal grid
    used = (hand >> 18) & 7  # nine hands with one slot left (every move a refill, by construction) and eight others
    one_left = [i for i in range(pos["n"]) if bin(int(used[i])).count("1") == 2 and not (int(hand[i]) >> 21) & 1]
    sel = one_left[:9] + list(range(4, 12))
    args = (1, 8, 128, 6)
    rows = P2.mixed_rows(17, "cpu")
    want = P2.call(*P2.to_tensors(board, hand, combo, "cpu", sel), rows, *args)
    got = P2.call(*P2.to_tensors(board, hand, combo, cuda, sel), rows.to(cuda), *args)
    P2.assert_equal(got, want, "deal grid cap")
    assert P2.leaf_kinds(want)[0] * 128 > 1000 and 17 * 8 * 128 > 1 << 14
    # 16,387 roots, above the 16,384 of the plan grid: the position set repeated, a row and a stream id each
    n = 16387
    rep = np.arange(n) % pos["n"]
    rows = P2.mixed_rows(n, "cpu")
    stream = torch.from_numpy((np.arange(n) % 1000).astype(np.int64))
    want = P2.call(*P2.to_tensors(board, hand, combo, "cpu", rep), rows, 1, 2, 1, 6, stream=stream)
    got = P2.call(*P2.to_tensors(board, hand, combo, cuda, rep), rows.to(cuda), 1, 2, 1, 6, stream=stream.to(cuda))
    P2.assert_equal(got, want, "plan grid cap")
    assert n > 1 << 14


def test_guard_words_each_output_alone_and_the_workspace(cuda, lib, pos):
    from runtime import kernels as K

    tb, th, tc = (t[:40].contiguous() for t in pos["t"])
    rows = pos["rows"][:40].contiguous()
    k, deals = 5, 3
    want = P2.call(tb, th, tc, rows, 2, k, deals, 13)
    need = K.plan2_work_bytes(40, k, deals)
    assert need == 40 * (192 * 12 + k * 28 + k * deals * 8) and need % 8 == 0
    work = torch.full((need + 128,), 0x5A, dtype=torch.uint8, device=cuda)
    bufs = {key: P2.guarded(40, k, deals, cuda, key) for key in P2.OUTPUTS}
    got = P2.call(tb, th, tc, rows, 2, k, deals, 13, out={key: v for key, (_, v) in bufs.items()}, work=work[64:64 + need])
    torch.cuda.synchronize()
    P2.assert_equal(got, want, "guarded")
    assert all(P2.guards_intact(b) for b, _ in bufs.values()) and P2.guards_intact(work)
    for key in P2.OUTPUTS:  # each output alone: the others live in the workspace
        buf, view = P2.guarded(40, k, deals, cuda, key)
        work.fill_(0x5A)
        P2.call(tb, th, tc, rows, 2, k, deals, 13, out={key: view}, work=work[64:64 + need])
        torch.cuda.synchronize()
        assert torch.equal(view, want[key]) and P2.guards_intact(buf) and P2.guards_intact(work), key
    with pytest.raises(Exception, match="work has"):
        P2.call(tb, th, tc, rows, 2, k, deals, 13, work=work[64:64 + need - 8])
    with pytest.raises(Exception, match="on cuda"):
        P2.call(tb, th, tc, rows.cpu(), 2, k, deals, 13)
    with pytest.raises(Exception, match="on cuda"):
        P2.call(tb, th, tc, rows, 2, k, deals, 13, work=torch.zeros(need, dtype=torch.uint8))
    with pytest.raises(Exception, match="on cuda"):
        P2.call(tb, th, tc, rows, 2, k, deals, 13, out={"action": torch.zeros(40, dtype=torch.int32)})


def test_graph_capture_from_the_first_call(cuda, lib, pos):
    """Captured on the very first call with these sizes, replayed after every input and output was rewritten; the seed
    is an argument by value, so the replay repeats the deals of the capture."""
    n, k, deals = 24, 4, 5
    src = [t[40:40 + n].clone() for t in pos["t"]]
    rows = pos["rows"][40:40 + n].clone()
    tb, th, tc = (torch.zeros_like(t) for t in src)
    live_rows = torch.zeros_like(rows)
    out = P2_outputs(n, k, deals, cuda)
    from runtime import kernels as K

    work = torch.empty(K.plan2_work_bytes(n, k, deals), dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            P2.call(tb, th, tc, live_rows, 3, k, deals, 99, out=out, work=work)
    for dst, s in zip((tb, th, tc, live_rows), (*src, rows)):
        dst.copy_(s)
    for v in out.values():
        v.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    want = P2.composed(*src, rows, 3, k, deals, 99)
    P2.assert_equal(out, want, "replay")
    assert P2.leaf_kinds(want)[0] > 10


def P2_outputs(n, k, deals, dev):
    from runtime import kernels as K

    return K.plan2_outputs(n, k, deals, dev, P2.OUTPUTS)
