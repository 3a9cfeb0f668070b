"""bb_playout_values(_pos) on the host backend against tests/_playout_ref.py: the oracle restatement on the tiny case
(depth 3 from its recorded answer, which one test holds to the oracle itself; depth 1-2 searched here), the composition
of the existing entry points on the 36 census boards and mid-game positions, hands == 1 against refill_values_ext, the
handle form, each output alone between guard words, every refusal (the same text from both libraries), n == 0 and the
Python argument rules.  Integer-exact, every output.  What a case is for is asserted from the reference's answers."""
import ctypes as C

import numpy as np
import pytest
import torch

import _playout_ref as PR

ERR_ARG = -1


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def golden():
    g = PR.tiny_golden()
    # what the tiny case is for, from the oracle's answers alone: all the endings, at more than one hand count
    survived, dead, cut, none = PR.endings(g[3])
    assert survived >= 8 and dead >= 3 and none >= 8 and cut == 0
    hands = g[3]["hands"]
    assert {1, 2, 3} <= set(hands.reshape(-1).tolist())
    assert ((g[3]["status"] & PR.PP.DEAD != 0) & (hands == 2)).any()   # a dead leaf behind a hand that was played out
    assert ((g[3]["status"] & PR.PP.REFILL != 0) & (hands == 3)).sum() >= 8
    assert (g[1]["plies"] <= 3).all() and (g[3]["plies"] == 9).any() and (g[3]["lines"] > 0).any()
    return g


@pytest.mark.slow
def test_the_recorded_answer_is_the_oracles(golden):
    """tests/golden/playout_tiny.json against the oracle searched now (half a minute: 120 hands three plies deep)."""
    want = PR.tiny_oracle()
    for h in (1, 2, 3):
        PR.assert_equal(golden[h], want[h], f"hands {h}")


@pytest.mark.parametrize("hands", [1, 2, 3])
def test_depth_3_against_the_oracle(host, golden, hands):
    board, rows, combo, stream = PR.tiny_tensors("cpu")
    got = PR.call(board, rows, 3, PR.TINY_PLAYOUTS, hands, PR.TINY_SEED, combo=combo, stream=stream)
    PR.assert_equal(got, golden[hands], f"hands {hands}")


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_1_and_2_against_the_oracle(host, depth):
    """A plan cut short by depth < 3 is no refill: every playout stops after its first hand, whatever ``hands``."""
    board, rows, combo, stream = PR.tiny_tensors("cpu")
    want = PR.oracle(PR.tiny_boards(), PR.TINY_WEIGHTS, depth, 4, 3, PR.TINY_SEED, combo=PR.TINY_COMBO,
                     stream=PR.TINY_STREAM)
    for hands in (1, 2, 3):
        got = PR.call(board, rows, depth, 4, hands, PR.TINY_SEED, combo=combo, stream=stream)
        PR.assert_equal(got, want[hands], f"depth {depth} hands {hands}")
    survived, dead, cut, none = PR.endings(want[3])
    assert survived == 0 and cut >= 8 and none >= 4 and (want[3]["hands"] == 1).all()
    played = want[3]["status"] != 0
    assert (want[3]["plies"][played] <= depth).all() and (want[3]["plies"][played] == depth).any()  # a dead leaf ends early


def census_and_midgame():
    """(boards u64, combo i32, stream i64): the 36 census boards and the mid-game positions of the refill tests."""
    import _census_ref as CR
    import _values_ext_ref as X

    boards, combo, _ = X.refill_boards()
    cb = CR.boards()
    assert len(cb) == 36
    bs = np.concatenate([cb, boards[len(PR.RV.FIXED_BOARDS):]])
    combo = np.concatenate([(np.arange(36) % 5).astype(np.int32), combo[len(PR.RV.FIXED_BOARDS):]])
    return bs, combo, (np.arange(len(bs)) // 2 + 5).astype(np.int64)


def mixed_rows(n, dev="cpu"):
    """int32 [n, 12]: shaped, zero-shape, anti-play and score-weighing rows in turn: both sides of the branch in a call."""
    kinds = PR.rows_of([PR.SHAPED, PR.PLAIN, PR.ANTI, PR.SCORED])
    return torch.stack([kinds[i % 4] for i in range(n)]).contiguous().to(dev)


@pytest.mark.parametrize("depth,hands", [(3, 3), (3, 1), (2, 2), (1, 3)])
def test_the_census_boards_against_the_composed_entry_points(host, depth, hands):
    bs, combo, stream = census_and_midgame()
    board, tc, ts = PR.board_tensor(bs), torch.from_numpy(combo), torch.from_numpy(stream)
    rows = mixed_rows(len(bs))
    want = PR.composed(board, rows, depth, 4, hands, 5, combo=tc, stream=ts)
    got = PR.call(board, rows, depth, 4, hands, 5, combo=tc, stream=ts)
    PR.assert_equal(got, want, f"depth {depth} hands {hands}")
    survived, dead, cut, none = PR.endings(want)
    if depth == 3:
        assert survived > 100 and dead >= 2 and none >= 4 and cut == 0
        if hands == 3:
            assert {1, 3} <= set(want["hands"].reshape(-1).tolist())  # the hand counts differ within the call
    else:
        assert survived == 0 and cut > 100
    one = PR.rows_of(PR.SHAPED)  # w_stride 0 against the same row repeated
    a = PR.call(board, one, depth, 4, hands, 5, combo=tc, stream=ts)
    b = PR.call(board, one.expand(len(bs), 12).contiguous(), depth, 4, hands, 5, combo=tc, stream=ts)
    PR.assert_equal(a, b, "shared row")


def test_one_hand_is_refill_values_ext(host):
    from runtime import kernels as K

    bs, combo, stream = census_and_midgame()
    board, tc, ts = PR.board_tensor(bs), torch.from_numpy(combo), torch.from_numpy(stream)
    rows = mixed_rows(len(bs))
    want = K.refill_values_ext(board, rows, 6, 9, combo=tc, stream=ts, want=("hand", "value"))
    got = PR.call(board, rows, 3, 6, 1, 9, combo=tc, stream=ts, want=("hand", "value", "hands"))
    assert torch.equal(got["hand"], want["hand"]) and torch.equal(got["value"], want["value"])
    assert (got["hands"] == 1).all()
    # NULL stream = i, NULL combo = 0
    ident = torch.arange(len(bs), dtype=torch.int64)
    a = PR.call(board, rows, 3, 3, 2, 9)
    b = PR.call(board, rows, 3, 3, 2, 9, combo=torch.zeros(len(bs), dtype=torch.int32), stream=ident)
    PR.assert_equal(a, b, "NULL columns")


def test_the_carried_combo_and_the_seed_wrap(host):
    """A row that weighs the score tells a carried combo from one reset between hands; seed 2^64 - 1 makes the second
    hand's key wrap to 0."""
    bs, combo, stream = census_and_midgame()
    board = PR.board_tensor(bs)
    rows = PR.rows_of(PR.SCORED)
    want = PR.composed(board, rows, 3, 4, 3, 5)
    wrong = PR.composed(board, rows, 3, 4, 3, 5, carry_combo=False)
    got = PR.call(board, rows, 3, 4, 3, 5)
    PR.assert_equal(got, want, "carried")
    assert (want["value"] != wrong["value"]).any() and (want["score"] != wrong["score"]).any()
    top = 2 ** 64 - 1  # ``composed`` keys hand 1 with (top + 1) mod 2^64 = 0
    few = board[:8].contiguous()
    got = PR.call(few, rows, 3, 4, 2, top)
    PR.assert_equal(got, PR.composed(few, rows, 3, 4, 2, top), "wrap")
    assert (got["hands"] == 2).any()


def test_the_handle_form_reads_the_live_state_and_changes_nothing(host):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(6, list(range(40, 46)), autoreset=False, device="cpu")
    env.reset()
    act = torch.zeros(6, dtype=torch.int32)
    for _ in range(8):
        env.plan_actions(act, PR.R.DEFAULT_WEIGHTS, 1)
        env.step(act)
    before = env.state()
    rows = mixed_rows(6)
    for stream in (None, torch.tensor([4, 4, 4, 9, 9, 1], dtype=torch.int64)):
        live = env.playout_values(rows, 3, 2, 21, stream=stream, want=PR.OUTPUTS)
        same = PR.call(PR.board_tensor(before["board"]), rows, 3, 3, 2, 21,
                       combo=torch.from_numpy(before["combo"].astype(np.int32)), stream=stream)
        PR.assert_equal(live, same, "handle")
    out = {"value": torch.zeros((6, 3), dtype=torch.int64)}
    assert env.playout_values(rows, 3, 2, 21, out=out) is out
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()
    assert K.PLAYOUT_MAX_HANDS == 256


def test_each_output_alone_and_nothing_beyond_it(host, golden):
    from runtime import lib as L

    n, m = 5, PR.TINY_PLAYOUTS
    boards, rows = PR.tiny_boards(), PR.rows_of(PR.TINY_WEIGHTS).numpy()
    combo, stream = PR.TINY_COMBO.copy(), PR.TINY_STREAM.astype(np.uint64)
    bufs = {k: np.zeros(n * m + 16, PR.DTYPES[k]) for k in PR.OUTPUTS}
    for wanted in [(k,) for k in PR.OUTPUTS] + [PR.OUTPUTS]:
        for v in bufs.values():
            v.view(np.uint8)[:] = 0x5A
        o = L.PlayoutOut(**{k: bufs[k][8:].ctypes.data for k in wanted})
        assert host.bb_playout_values_pos(boards.ctypes.data, combo.ctypes.data, stream.ctypes.data, n,
                                          rows.ctypes.data, 1, 3, m, 3, PR.TINY_SEED, C.byref(o), None) == 0
        for k, v in bufs.items():
            raw = v.view(np.uint8).reshape(len(v), -1)
            assert (raw[:8] == 0x5A).all() and (raw[8 + n * m:] == 0x5A).all(), k
            if k in wanted:
                assert v[8:8 + n * m].reshape(n, m).tolist() == golden[3][k].tolist(), k
            else:
                assert (raw == 0x5A).all(), k


FAKE = 0x1000
RULES = [(dict(w=None), "weight rows are NULL"), (dict(stride=2), "w_stride must be 0 or 1"),
         (dict(stride=-1), "w_stride must be 0 or 1"), (dict(out=None), "out is NULL"),
         (dict(out={}), "all nine outputs are NULL"), (dict(depth=0), "depth must be 1..3"),
         (dict(depth=4), "depth must be 1..3"), (dict(playouts=0), "playouts must be 1..1024"),
         (dict(playouts=1025), "playouts must be 1..1024"), (dict(hands=0), "hands must be 1..256"),
         (dict(hands=257), "hands must be 1..256")]
POS_REFUSALS = [(dict(board=None), "board is NULL"), (dict(n=-1), "n is negative")] + RULES


def _call(backend, kw, handle=None, env_form=False):
    from runtime import lib as L

    a = {"board": FAKE, "n": 4, "w": FAKE, "stride": 1, "depth": 3, "playouts": 4, "hands": 2,
         "out": dict(value=FAKE), **kw}
    o = L.PlayoutOut(**a["out"]) if a["out"] is not None else None
    rest = (a["w"], a["stride"], a["depth"], a["playouts"], a["hands"], 1, C.byref(o) if o is not None else None, None)
    if env_form:
        return backend.bb_playout_values(handle, None, *rest)
    return backend.bb_playout_values_pos(a["board"], None, None, a["n"], *rest)


@pytest.mark.parametrize("kw,text", POS_REFUSALS, ids=[f"{i}-{t}" for i, (_, t) in enumerate(POS_REFUSALS)])
def test_pos_rules_are_one_set_for_both_backends(lib, host, kw, text):
    """Refused with BB_ERR_ARG before any HIP call (so libbbvec.so answers without a GPU), the same text from both."""
    from runtime import lib as L

    for backend in (lib, host):
        assert _call(backend, kw) == ERR_ARG
        assert L.last_error(lib=backend) == f"bb_playout_values_pos: {text}"


@pytest.mark.parametrize("kw,text", RULES, ids=[f"{i}-{t}" for i, (_, t) in enumerate(RULES)])
def test_handle_rules_on_the_host_backend(host, kw, text):
    from runtime import lib as L
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    env.reset()
    assert _call(host, kw, env.handle, env_form=True) == ERR_ARG
    assert L.last_error(env.handle, host) == f"bb_playout_values: {text}"
    assert _call(host, {}, None, env_form=True) == ERR_ARG  # a NULL handle
    env.close()


def test_no_boards_is_accepted_and_does_nothing(lib, host):
    for backend in (lib, host):
        for k in PR.OUTPUTS:
            assert _call(backend, dict(n=0, out={k: FAKE})) == 0
    got = PR.call(torch.zeros(0, dtype=torch.int64), PR.rows_of(PR.PLAIN), 3, 3, 2, 1)
    assert all(t.shape == (0, 3) for t in got.values()) and set(got) == set(PR.OUTPUTS)


def test_the_bounds_of_playouts_and_hands(host):
    b = PR.board_tensor(np.zeros(1, np.uint64))
    rows = PR.rows_of(PR.PLAIN)
    got = PR.call(b, rows, 1, 1024, 1, 5, want=("hands", "plies"))
    assert got["hands"].shape == (1, 1024) and (got["plies"] == 1).all()
    got = PR.call(b, rows, 3, 1, 256, 5, want=("hands", "plies", "status"))
    assert got["hands"].tolist() == [[256]] and got["plies"].tolist() == [[768]] and int(got["status"]) & PR.PP.REFILL


def test_python_argument_rules(host):
    from runtime import kernels as K
    from runtime import lib as L

    b = PR.board_tensor(PR.tiny_boards())
    rows = PR.rows_of(PR.TINY_WEIGHTS)
    for bad in (b.to(torch.int32), b.reshape(5, 1), b.numpy()):
        with pytest.raises(L.BBNativeError, match="board must be a contiguous torch.int64 tensor of shape"):
            K.playout_values(bad, rows, 2, 2, 1)
    for playouts in (0, 1025, 2.0):
        with pytest.raises(L.BBNativeError, match="playouts must be 1..1024"):
            K.playout_values(b, rows, playouts, 2, 1)
    for hands in (0, 257, 2.0):
        with pytest.raises(L.BBNativeError, match="hands must be 1..256"):
            K.playout_values(b, rows, 2, hands, 1)
    for depth in (0, 4):
        with pytest.raises(L.BBNativeError, match="depth must be 1..3"):
            K.playout_values(b, rows, 2, 2, 1, depth=depth)
    with pytest.raises(L.BBNativeError, match="rows must be a contiguous"):
        K.playout_values(b, rows[:3].contiguous(), 2, 2, 1)
    with pytest.raises(L.BBNativeError, match="combo must be a contiguous"):
        K.playout_values(b, rows, 2, 2, 1, combo=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(L.BBNativeError, match="stream must be a contiguous"):
        K.playout_values(b, rows, 2, 2, 1, stream=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.playout_values(b, rows, 2, 2, 1, want=("value", "plan"))
    with pytest.raises(L.BBNativeError, match="at least one of value"):
        K.playout_values(b, rows, 2, 2, 1, out={})
    with pytest.raises(L.BBNativeError, match="score must be a contiguous"):
        K.playout_values(b, rows, 2, 2, 1, out={"score": torch.zeros((5, 2), dtype=torch.int32)})
    out = {"plies": torch.zeros((5, 2), dtype=torch.int32)}
    assert K.playout_values(b, rows, 2, 2, 1, out=out) is out
    assert set(K.playout_values(b, rows, 2, 2, 1)) == {"value"}
