"""bb_plan_values_ext / bb_refill_values_ext on the host backend (libbbvec_host.so) and their Python surface, on the
CPU, no GPU involved.

The references are tests/_values_ext_ref.py's, which call none of the new entry points.  Zero shape weights are held
to the existing ``plan_values`` / ``refill_values`` on every output, so the new entry points cannot pass by agreeing
only with themselves.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _refill_values_ref as RV
import _values_ext_ref as X

CPU = torch.device("cpu")
NAMES = X.NAMES
PV_KEYS = ("q", "rest", "leaves", "safe")
RV_KEYS = ("hand", "value", "attempts")


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def ref(host):
    return R.reference()


def _base(w):
    from runtime import lib as L

    return {k: v for k, v in w.items() if k in L.GREEDY_FIELDS}


def _pv(cols, rows, depth, **kw):
    from runtime import kernels as K

    return K.plan_values_ext(cols[0], cols[1], rows, depth, combo=cols[2], **kw)


def _same(got, want, keys, what):
    for k in keys:
        assert torch.equal(got[k], want[k]), (what, k, torch.nonzero(got[k] != want[k])[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------
# per-action values
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_plan_values_ext_equals_the_reference(ref, depth):
    from runtime import kernels as K

    idx, want = X.reference_values(depth, depth < 3)  # depth 3: the small trees
    assert len(idx) == ref["n"] if depth < 3 else 40 <= len(idx) < ref["n"]
    cols = R.tensors(ref, CPU, idx)[:3]
    for name, w in X.SETS.items():
        X.check(_pv(cols, K.eval_rows(w), depth), want, name, what=f"depth {depth}")
    assert all(X.pairs_changed(want, k) >= 5 for k in NAMES if k != "zero4")


@pytest.mark.slow
def test_plan_values_ext_equals_the_reference_on_the_whole_set_at_depth_3(ref):
    from runtime import kernels as K

    idx, want = X.reference_values(3, True)  # asserts the issue's change counts itself
    cols = R.tensors(ref, CPU)[:3]
    for name, w in X.SETS.items():
        X.check(_pv(cols, K.eval_rows(w), 3), want, name, what="depth 3, whole set")


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_zero_shape_weights_equal_plan_values_on_every_output(ref, depth):
    from _weights_each import SETS as BASES
    from runtime import kernels as K

    n = ref["n"]
    cols = R.tensors(ref, CPU)[:3]
    for base in BASES + [X.SETS["zero4"]]:
        want = K.plan_values(cols[0], cols[1], _base(base), depth, combo=cols[2])
        _same(_pv(cols, K.eval_rows(base), depth), want, PV_KEYS, f"shared row, depth {depth}")
        _same(_pv(cols, K.eval_rows(base, n=n), depth), want, PV_KEYS, f"own rows, depth {depth}")


def test_stride_0_equals_replicated_rows_and_interleaved_rows_equal_per_set_calls(ref):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    n = ref["n"]
    cols = R.tensors(ref, CPU)[:3]
    per_set = [_pv(cols, K.eval_rows(X.SETS[k]), 2) for k in NAMES]
    for k, shared in zip(NAMES, per_set):
        _same(_pv(cols, K.eval_rows(X.SETS[k], n=n), 2), shared, PV_KEYS, f"replicated {k}")
    which = torch.as_tensor((np.arange(n) + 3) % len(NAMES))
    rows = K.eval_rows([X.SETS[NAMES[j]] for j in which.tolist()])
    want = {k: torch.stack([r[k] for r in per_set])[which, torch.arange(n)] for k in PV_KEYS}
    _same(_pv(cols, rows, 2), want, PV_KEYS, "interleaved rows")
    assert any(not torch.equal(per_set[0]["q"], r["q"]) for r in per_set[1:])
    for r in per_set[1:]:  # safe and leaves do not depend on the weights
        _same(r, per_set[0], ("leaves", "safe"), "weight-free outputs")

    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    _same(env.plan_values_ext(rows, 2), want, PV_KEYS, "handle form, own rows")
    _same(env.plan_values_ext(K.eval_rows(X.SETS["all"]), 2), per_set[NAMES.index("all")], PV_KEYS, "handle, shared")
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before), "the handle form changed the state"
    env.close()


def test_plan_values_ext_agrees_with_plan_actions_ext(ref):
    """max_a q, its lowest arg-max, the decoded rest and the sum of leaves are bb_plan_actions_ext's answers."""
    from runtime import kernels as K

    cols = R.tensors(ref, CPU)[:3]
    for name in ("all", "mixed"):
        rows = K.eval_rows(X.SETS[name])
        pv = _pv(cols, rows, 2)
        pa = K.plan_actions_ext(cols[0], cols[1], rows, 2, combo=cols[2], want_plan=True, want_leaves=True)
        found = pa["leaves"] > 0
        a = pv["q"].argmax(dim=1)
        assert torch.equal(pv["q"].max(dim=1).values, pa["value"]) and torch.equal(pv["leaves"].sum(dim=1).int(), pa["leaves"])
        assert torch.equal(torch.where(found, a, torch.zeros_like(a)).int(), pa["action"])
        a2, a3 = K.unpack_rest(pv["rest"][torch.arange(len(a)), a])
        assert torch.equal(a2[found].int(), pa["plan"][found, 1]) and torch.equal(a3[found].int(), pa["plan"][found, 2])


def test_positions_without_a_legal_move(ref):
    from _weights_each import no_action_positions
    from runtime import kernels as K

    board, hand = no_action_positions(ref)
    rows = K.eval_rows([X.SETS[NAMES[i % len(NAMES)]] for i in range(8)])
    for depth in (1, 2, 3):
        for r in (rows, K.eval_rows(X.SETS["mixed"])):
            got = K.plan_values_ext(board, hand, r, depth)
            assert (got["q"] == R.INT64_MIN).all() and (got["rest"] == -1).all()
            assert (got["leaves"] == 0).all() and (got["safe"] == 0).all()


@pytest.mark.parametrize("key", PV_KEYS)
def test_each_plan_values_output_alone_between_guard_words(ref, key):
    from runtime import kernels as K

    n = 9
    cols = tuple(t[:n].contiguous() for t in R.tensors(ref, CPU)[:3])
    rows = K.eval_rows([X.SETS[NAMES[i % len(NAMES)]] for i in range(n)])
    whole = _pv(cols, rows, 2)
    dt, width = K.PLAN_VALUE_OUTPUTS[key]
    buf = torch.full((n * width + 16,), -77, dtype=dt)
    got = _pv(cols, rows, 2, out={key: buf[8:8 + n * width].view(n, width)})
    assert set(got) == {key} and torch.equal(got[key], whole[key])
    assert (buf[:8] == -77).all() and (buf[8 + n * width:] == -77).all()


# ---------------------------------------------------------------------------------------------------------------
# dealt next-hand values
# ---------------------------------------------------------------------------------------------------------------
def _refill_cols():
    boards, combo, stream = X.refill_boards()
    return RV.board_tensor(boards), torch.from_numpy(combo.copy()), torch.from_numpy(stream.copy())


@pytest.mark.parametrize("deals,depth", X.REFILL_CASES)
def test_refill_values_ext_equals_the_reference(host, deals, depth):
    from runtime import kernels as K

    want = X.reference_refill(deals, depth)
    board, combo, stream = _refill_cols()
    n = board.numel()
    base = K.refill_values(board, _base(X.SETS["zero4"]), deals, X.REFILL_SEED, combo=combo, stream=stream, depth=depth,
                           want=RV_KEYS)
    assert np.array_equal(RV.as_u32(base["hand"]), want["hand"]) and np.array_equal(base["attempts"].numpy(), want["attempts"])
    per_set = {}
    for name, w in X.SETS.items():
        got = K.refill_values_ext(board, K.eval_rows(w), deals, X.REFILL_SEED, combo=combo, stream=stream, depth=depth,
                                  want=RV_KEYS)
        _same(got, base, ("hand", "attempts"), f"{name}: the deal reads no weights")
        assert np.array_equal(got["value"].numpy(), want["value"][name]), (name, deals, depth)
        per_set[name] = got["value"]
    assert torch.equal(per_set["zero4"], base["value"])
    # per-board rows: every deal of board i under board i's row
    which = (np.arange(n) + 2) % len(NAMES)
    got = K.refill_values_ext(board, K.eval_rows([X.SETS[NAMES[j]] for j in which]), deals, X.REFILL_SEED, combo=combo,
                              stream=stream, depth=depth)
    for i in range(n):
        assert torch.equal(got["value"][i], per_set[NAMES[which[i]]][i]), i
    # two boards with one stream id meet the same draws before the acceptance test
    assert stream[0] == stream[1]


def test_zero_shape_weights_equal_refill_values_and_the_handle_form(ref):
    from _weights_each import SETS as BASES
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    board, combo, stream = _refill_cols()
    n = board.numel()
    for base in BASES + [X.SETS["zero4"]]:
        want = K.refill_values(board, _base(base), 3, 11, combo=combo, stream=stream, depth=2, want=RV_KEYS)
        for rows in (K.eval_rows(base), K.eval_rows(base, n=n)):
            _same(K.refill_values_ext(board, rows, 3, 11, combo=combo, stream=stream, depth=2, want=RV_KEYS), want,
                  RV_KEYS, "zero shape weights")
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    env.set_state(board=X.refill_boards()[0], combo=X.refill_boards()[1])
    before = env.state()
    rows = K.eval_rows([X.SETS[NAMES[i % len(NAMES)]] for i in range(n)])
    want = K.refill_values_ext(board, rows, 3, 11, combo=combo, stream=stream, depth=2, want=RV_KEYS)
    _same(env.refill_values_ext(rows, 3, 11, stream=stream, depth=2, want=RV_KEYS), want, RV_KEYS, "handle form")
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before), "the handle form changed the state"
    env.close()


def test_a_dealt_hand_without_a_first_move_gets_base_dead_alone(host):
    from runtime import kernels as K

    board = RV.board_tensor([RV.FIXED_BOARDS[RV.FULL]] * 2)
    rows = K.eval_rows([X.SETS["all"], X.SETS["mixed"]])
    got = K.refill_values_ext(board, rows, 4, 3, depth=3, want=RV_KEYS)
    assert (got["attempts"] == -100).all()
    assert (got["value"][0] == X.SETS["all"]["dead"]).all() and (got["value"][1] == X.SETS["mixed"]["dead"]).all()


@pytest.mark.parametrize("key", RV_KEYS)
def test_each_refill_output_alone_between_guard_words(host, key):
    from runtime import kernels as K

    board, combo, stream = _refill_cols()
    n, m = board.numel(), 3
    rows = K.eval_rows([X.SETS[NAMES[i % len(NAMES)]] for i in range(n)])
    whole = K.refill_values_ext(board, rows, m, 5, combo=combo, stream=stream, depth=2, want=RV_KEYS)
    buf = torch.full((n * m + 16,), -77, dtype=K.REFILL_VALUE_OUTPUTS[key])
    got = K.refill_values_ext(board, rows, m, 5, combo=combo, stream=stream, depth=2,
                              out={key: buf[8:8 + n * m].view(n, m)})
    assert set(got) == {key} and torch.equal(got[key], whole[key])
    assert (buf[:8] == -77).all() and (buf[8 + n * m:] == -77).all()


# ---------------------------------------------------------------------------------------------------------------
# the Python argument rules
# ---------------------------------------------------------------------------------------------------------------
def test_python_argument_rules(ref):
    from runtime import kernels as K
    from runtime.lib import BBNativeError

    cols = tuple(t[:8].contiguous() for t in R.tensors(ref, CPU)[:3])
    good = K.eval_rows({}, n=8)
    bad = {"dtype": good.long(), "rows": K.eval_rows({}, n=3), "width": torch.zeros((8, 8), dtype=torch.int32),
           "contiguity": torch.zeros((8, 24), dtype=torch.int32)[:, ::2], "not a tensor": [[0] * 12] * 8}
    for what, r in bad.items():
        with pytest.raises(BBNativeError, match=r"plan_values_ext: rows must be a contiguous torch.int32 \[1, 12\] or \[8, 12\]"):
            _pv(cols, r, 2)
        with pytest.raises(BBNativeError, match=r"refill_values_ext: rows must be a contiguous torch.int32 \[1, 12\] or \[8, 12\]"):
            K.refill_values_ext(cols[0], r, 2, 1)
    with pytest.raises(BBNativeError, match="depth must be 1..3"):
        _pv(cols, good, 4)
    with pytest.raises(BBNativeError, match="unknown outputs"):
        _pv(cols, good, 2, out={"value": torch.zeros(8, dtype=torch.int64)})
    with pytest.raises(ValueError, match="unknown plan_values outputs"):
        _pv(cols, good, 2, want=("q", "value"))
    with pytest.raises(BBNativeError, match="at least one of"):
        _pv(cols, good, 2, out={})
    with pytest.raises(BBNativeError, match="prev must be a contiguous"):
        K.plan_values_ext(cols[0], cols[1], good, 2, prev=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(BBNativeError, match="deals must be 1..1024"):
        K.refill_values_ext(cols[0], good, 0, 1)
    with pytest.raises(BBNativeError, match="depth must be 1..3"):
        K.refill_values_ext(cols[0], good, 2, 1, depth=0)
    with pytest.raises(BBNativeError, match="board must be a contiguous torch.int64"):
        K.refill_values_ext(cols[1], good, 2, 1)
    with pytest.raises(BBNativeError, match="stream must be a contiguous"):
        K.refill_values_ext(cols[0], good, 2, 1, stream=torch.zeros(8, dtype=torch.int32))
    empty = K.refill_values_ext(torch.zeros(0, dtype=torch.int64), K.eval_rows({}), 2, 1)
    assert empty["value"].shape == (0, 2)
