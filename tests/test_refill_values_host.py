"""Dealt next-hand values on the host backend (bb_refill_values / bb_refill_values_pos of libbbvec_host.so), on the
CPU (no GPU involved), against tests/_refill_values_ref.py, which calls neither: hand, value and attempts of the fixed
case at every depth, the combo's effect, common random numbers under one stream id, agreement with the refill census,
the handle form, each output alone between guard words, the bounds of ``deals``, every refusal (the same text from
both libraries), n == 0 and the Python argument rules.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _refill_values_ref as RV

ERR_ARG = -1
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SCORED = {"lines": 10, "score": 1, "holes": -3, "filled": -1, "dead": -5000}  # the score weight makes the combo count


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_host_equals_the_reference_on_the_fixed_case(host, depth):
    from runtime import kernels as K

    ref = RV.fixed(depth)
    got = K.refill_values(RV.board_tensor(RV.FIXED_BOARDS), RV.WEIGHTS, RV.FIXED_DEALS, RV.FIXED_SEED, depth=depth,
                          want=("hand", "value", "attempts"))
    assert got["hand"].dtype == torch.int32 and got["value"].dtype == torch.int64
    assert all(t.shape == (5, RV.FIXED_DEALS) for t in got.values())
    assert got["attempts"].tolist() == ref["attempts"].tolist()
    assert RV.as_u32(got["hand"]).tolist() == ref["hand"].tolist()
    assert got["value"].tolist() == ref["value"].tolist()
    assert (got["value"][RV.FULL] == RV.WEIGHTS["dead"]).all()  # no legal first move: the dead weight


def test_the_combo_is_carried_into_the_value(host):
    """A board one cell short of a full row: a hand that fills it clears a line, and the score of that move grows
    with the streak it continues."""
    from runtime import kernels as K

    boards = np.array([0x7F, 0x7F7F], np.uint64)
    ref0 = RV.refill_values(boards, 8, 3, 3, SCORED, combo=[0, 0])
    ref5 = RV.refill_values(boards, 8, 3, 3, SCORED, combo=[5, 5])
    assert (ref0["hand"] == ref5["hand"]).all() and (ref0["value"] != ref5["value"]).any()
    b = RV.board_tensor(boards)
    for combo, ref in ((0, ref0), (5, ref5)):
        got = K.refill_values(b, SCORED, 8, 3, combo=torch.full((2,), combo, dtype=torch.int32))
        assert got["value"].tolist() == ref["value"].tolist()
    assert K.refill_values(b, SCORED, 8, 3)["value"].tolist() == ref0["value"].tolist()  # no combo column: 0


def test_one_stream_id_gives_common_random_numbers(host):
    from runtime import kernels as K

    boards = RV.FIXED_BOARDS[[RV.EMPTY, RV.CHECKER_ROW7_EMPTY, RV.ONE_HOLE, RV.EMPTY]]
    stream = torch.tensor([7, 7, 7, 8], dtype=torch.int64)
    got = K.refill_values(RV.board_tensor(boards), RV.WEIGHTS, 32, 11, stream=stream, depth=1, want=("hand", "attempts"))
    ref_hand, ref_at = RV.deal(boards, 32, 11, stream.numpy())
    assert RV.as_u32(got["hand"]).tolist() == ref_hand.tolist() and got["attempts"].tolist() == ref_at.tolist()
    hand, at = got["hand"], got["attempts"]
    same = 0
    for x, y in ((0, 1), (0, 2), (1, 2)):
        both = at[x] == at[y]
        same += int(both.sum())
        assert torch.equal(hand[x][both], hand[y][both])
    assert same >= 3
    assert not torch.equal(hand[0], hand[3])  # another stream id, other draws


def test_accepted_hands_are_the_census_solvable_hands(host):
    from runtime import kernels as K

    b = RV.board_tensor(RV.FIXED_BOARDS)
    got = K.refill_values(b, RV.WEIGHTS, RV.FIXED_DEALS, RV.FIXED_SEED, depth=1, want=("hand", "attempts"))
    words = K.refill_census(b, want=("solvable",))["solvable"].numpy().view(np.uint64)
    hand, at = RV.as_u32(got["hand"]).astype(np.int64), got["attempts"].numpy()
    a, bb, c = hand & 63, (hand >> 6) & 63, (hand >> 12) & 63
    assert (hand >> 18 == 0).all() and max(a.max(), bb.max(), c.max()) < 37
    bit = (words[np.arange(5)[:, None], a, bb] >> c.astype(np.uint64)) & np.uint64(1)
    assert ((bit == 1) == (at > 0)).all()
    assert ((at >= 1) & (at <= 100) | (at == -100)).all()


def test_handle_form_equals_pos_form_and_changes_nothing(host):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(5, [1, 2, 3, 4, 5], autoreset=False, device="cpu")
    env.reset()
    combo = np.array([0, 1, 2, 3, 4], np.int32)
    env.set_state(board=RV.FIXED_BOARDS, combo=combo)
    before = env.state()
    for stream in (None, torch.tensor([4, 4, 4, 9, 9], dtype=torch.int64)):
        want = K.refill_values(RV.board_tensor(RV.FIXED_BOARDS), SCORED, 4, 21, combo=torch.from_numpy(combo),
                               stream=stream, depth=2, want=("hand", "value", "attempts"))
        got = env.refill_values(SCORED, 4, 21, stream=stream, depth=2, want=("hand", "value", "attempts"))
        for k in want:
            assert torch.equal(got[k], want[k]), k
    out = {"value": torch.zeros((5, 4), dtype=torch.int64)}
    assert env.refill_values(SCORED, 4, 21, depth=2, out=out) is out
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


def test_each_output_alone_and_nothing_beyond_it(host):
    from runtime import lib as L

    ref = RV.fixed(2)
    n, m = 5, RV.FIXED_DEALS
    w = L.greedy_weights(RV.WEIGHTS)
    bufs = {"hand": np.zeros(n * m + 16, np.uint32), "value": np.zeros(n * m + 16, np.int64),
            "attempts": np.zeros(n * m + 16, np.int32)}
    guard = {"hand": GUARD32, "value": GUARD64, "attempts": GUARD32}
    for wanted in (("hand",), ("value",), ("attempts",), ("hand", "value", "attempts")):
        for k, v in bufs.items():
            v[:] = guard[k]
        o = L.RefillValuesOut(**{k: bufs[k][8:].ctypes.data for k in wanted})
        assert host.bb_refill_values_pos(RV.FIXED_BOARDS.ctypes.data, None, None, n, C.byref(w), 2, m, RV.FIXED_SEED,
                                         C.byref(o), None) == 0
        for k, v in bufs.items():
            assert (v[:8] == guard[k]).all() and (v[8 + n * m:] == guard[k]).all(), k
            if k in wanted:
                assert v[8:8 + n * m].reshape(n, m).tolist() == ref[k].tolist(), k
            else:
                assert (v == guard[k]).all(), k


def test_the_bounds_of_deals(host):
    from runtime import kernels as K
    from runtime import lib as L

    b = RV.board_tensor(RV.FIXED_BOARDS[:1])
    for deals in (1, 1024):
        got = K.refill_values(b, RV.WEIGHTS, deals, 5, depth=1, want=("hand", "attempts"))
        assert got["attempts"].shape == (1, deals) and (got["attempts"] == 1).all()
        ref_hand, _ = RV.deal(RV.FIXED_BOARDS[:1], min(deals, 4), 5)
        assert RV.as_u32(got["hand"])[:, :4].tolist() == ref_hand.tolist()
    w = L.greedy_weights(RV.WEIGHTS)
    one = np.zeros(1, np.int32)
    o = L.RefillValuesOut(attempts=one.ctypes.data)
    for deals in (0, 1025, -1):
        assert host.bb_refill_values_pos(RV.FIXED_BOARDS.ctypes.data, None, None, 1, C.byref(w), 1, deals, 5,
                                         C.byref(o), None) == ERR_ARG
        assert L.last_error(lib=host) == "bb_refill_values_pos: deals must be 1..1024"


FAKE = 0x1000
RULES = [(dict(w=False), "weights are NULL"), (dict(out=None), "out is NULL"),
         (dict(out={}), "all three outputs are NULL"), (dict(depth=0), "depth must be 1..3"),
         (dict(depth=4), "depth must be 1..3"), (dict(deals=0), "deals must be 1..1024"),
         (dict(deals=1025), "deals must be 1..1024")]
POS_REFUSALS = [(dict(board=None), "board is NULL"), (dict(n=-1), "n is negative")] + RULES


def _call(backend, kw, handle=None, env_form=False):
    from runtime import lib as L

    a = {"board": FAKE, "n": 4, "w": True, "depth": 3, "deals": 4, "out": dict(value=FAKE), **kw}
    w = L.greedy_weights({"lines": 1}) if a["w"] else None
    o = L.RefillValuesOut(**a["out"]) if a["out"] is not None else None
    rest = (C.byref(w) if w is not None else None, a["depth"], a["deals"], 1, C.byref(o) if o is not None else None,
            None)
    if env_form:
        return backend.bb_refill_values(handle, None, *rest)
    return backend.bb_refill_values_pos(a["board"], None, None, a["n"], *rest)


@pytest.mark.parametrize("kw,text", POS_REFUSALS, ids=[f"{i}-{t}" for i, (_, t) in enumerate(POS_REFUSALS)])
def test_pos_rules_are_one_set_for_both_backends(lib, host, kw, text):
    """Refused with BB_ERR_ARG before any HIP call (so libbbvec.so answers without a GPU), the same text from both."""
    from runtime import lib as L

    for backend in (lib, host):
        assert _call(backend, kw) == ERR_ARG
        assert L.last_error(lib=backend) == f"bb_refill_values_pos: {text}"


@pytest.mark.parametrize("kw,text", RULES, ids=[f"{i}-{t}" for i, (_, t) in enumerate(RULES)])
def test_handle_rules_on_the_host_backend(host, kw, text):
    from runtime import lib as L
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    env.reset()
    assert _call(host, kw, env.handle, env_form=True) == ERR_ARG
    assert L.last_error(env.handle, host) == f"bb_refill_values: {text}"
    assert _call(host, {}, None, env_form=True) == ERR_ARG  # a NULL handle
    env.close()


def test_no_boards_is_accepted_and_does_nothing(lib, host):
    from runtime import kernels as K

    for backend in (lib, host):
        for out in (dict(hand=FAKE), dict(value=FAKE), dict(attempts=FAKE)):
            assert _call(backend, dict(n=0, out=out)) == 0
    got = K.refill_values(torch.zeros(0, dtype=torch.int64), RV.WEIGHTS, 3, 1, want=("hand", "value", "attempts"))
    assert all(t.shape == (0, 3) for t in got.values())


def test_python_argument_rules(host):
    from runtime import kernels as K
    from runtime import lib as L

    b = RV.board_tensor(RV.FIXED_BOARDS)
    for bad in (b.to(torch.int32), b.reshape(5, 1), torch.stack([b, b], dim=1)[:, 0], b.numpy()):
        with pytest.raises(L.BBNativeError, match="board must be a contiguous torch.int64 tensor of shape"):
            K.refill_values(bad, RV.WEIGHTS, 2, 1)
    for deals in (0, 1025, 2.0):
        with pytest.raises(L.BBNativeError, match="deals must be 1..1024"):
            K.refill_values(b, RV.WEIGHTS, deals, 1)
    for depth in (0, 4):
        with pytest.raises(L.BBNativeError, match="depth must be 1..3"):
            K.refill_values(b, RV.WEIGHTS, 2, 1, depth=depth)
    with pytest.raises(L.BBNativeError, match="combo must be a contiguous"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, combo=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(L.BBNativeError, match="combo must be a contiguous"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, combo=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(L.BBNativeError, match="stream must be a contiguous"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, stream=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, want=("value", "plan"))
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, out={"plan": torch.zeros((5, 2), dtype=torch.int32)})
    with pytest.raises(L.BBNativeError, match="at least one of hand, value, attempts"):
        K.refill_values(b, RV.WEIGHTS, 2, 1, out={})
    for k, t in (("value", torch.zeros((5, 2), dtype=torch.int32)), ("value", torch.zeros((5, 3), dtype=torch.int64)),
                 ("hand", torch.zeros((5, 4), dtype=torch.int32)[:, ::2]),
                 ("attempts", torch.zeros((4, 2), dtype=torch.int32))):
        with pytest.raises(L.BBNativeError, match=f"{k} must be a contiguous"):
            K.refill_values(b, RV.WEIGHTS, 2, 1, out={k: t})
    with pytest.raises(ValueError):
        K.refill_values(b, {"lines": 1, "luck": 2}, 2, 1)
    out = {"attempts": torch.zeros((5, 2), dtype=torch.int32)}
    assert K.refill_values(b, RV.WEIGHTS, 2, RV.FIXED_SEED, out=out) is out
    assert out["attempts"].tolist() == RV.fixed(1)["attempts"][:, :2].tolist()
    assert set(K.refill_values(b, RV.WEIGHTS, 2, 1, depth=1)) == {"value"}
