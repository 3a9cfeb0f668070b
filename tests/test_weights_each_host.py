"""One row of weights per position on the host backend (bb_greedy_actions_each / bb_plan_actions_each of
libbbvec_host.so), on the CPU, no GPU involved.  The contract is one sentence -- position i's outputs are those the
uniform entry point returns for it with w = d_w[i] -- so the reference is the uniform calls themselves, which
tests/test_plan_host.py and tests/test_afterstates_host.py hold to the oracle: four weight sets dealt round-robin
over the 92 positions of tests/_afterstates_ref.py, gathered by set.  Then equal rows, the handle forms, positions
without a legal action, NULL optional outputs, every refusal rule from both libraries, and ``weight_rows``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _afterstates_ref as R
from _weights_each import BIG, CPU, KEYS, SETS, gathered, mixed_rows, no_action_positions

FAKE = 0x1000  # a non-NULL pointer no refused call dereferences


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def ref(host):
    return R.reference()


def test_weight_rows_layout_and_checks(host):
    from runtime import kernels as K
    from runtime import lib as L

    w = {k: 10 + j for j, k in enumerate(L.GREEDY_FIELDS)}
    one = K.weight_rows(w)
    assert one.dtype == torch.int32 and one.is_contiguous() and one.tolist() == [list(range(10, 18))]
    s = L.greedy_weights(w)  # the struct's field order, read back as raw int32
    assert list((C.c_int32 * 8).from_buffer_copy(bytes(s))) == one[0].tolist()
    assert K.weight_rows({"holes": -3}, n=3).tolist() == [[0, 0, -3, 0, 0, 0, 0, 0]] * 3
    two = K.weight_rows([{"lines": BIG}, {"refill": -BIG}])
    assert two.tolist() == [[BIG, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, -BIG]]
    with pytest.raises(ValueError, match="unknown greedy weights"):
        K.weight_rows({"linez": 1})
    with pytest.raises(ValueError, match="unknown greedy weights"):
        K.weight_rows([{}, {"hole": 1}])
    with pytest.raises(ValueError):
        K.weight_rows([{}, {}], n=3)


def test_bad_rows_tensor_is_refused_by_name(ref):
    from runtime import kernels as K
    from runtime.lib import BBNativeError

    board, hand, combo, _ = R.tensors(ref, CPU, np.arange(4))
    good = K.weight_rows({}, n=4)
    bad = {"dtype": good.long(), "rows": K.weight_rows({}, n=3), "width": torch.zeros((4, 7), dtype=torch.int32),
           "contiguity": torch.zeros((4, 16), dtype=torch.int32)[:, ::2], "not a tensor": [[0] * 8] * 4}
    for what, rows in bad.items():
        for call in (lambda r: K.plan_actions_each(board, hand, r, 2, combo=combo),
                     lambda r: K.greedy_actions_each(board, hand, r, combo=combo)):
            with pytest.raises(BBNativeError, match=r"rows must be a contiguous torch.int32 \[4, 8\]"):
                call(rows)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_plan_each_equals_uniform_gathered_by_set(ref, depth):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU)
    rows, which = mixed_rows(ref["n"])
    uniform = [K.plan_actions(board, hand, w, depth, combo=combo, want_plan=True, want_leaves=True) for w in SETS]
    want = gathered(uniform, which)
    got = K.plan_actions_each(board, hand, rows, depth, combo=combo, want_plan=True, want_leaves=True)
    for k in KEYS:
        bad = torch.nonzero((got[k] != want[k]).reshape(ref["n"], -1).any(dim=1)).flatten()[:4]
        assert bad.numel() == 0, (k, depth, bad.tolist(), got[k][bad].tolist(), want[k][bad].tolist())
    # the sets disagree somewhere, so a call that read one row for everyone would have failed above
    assert any(not torch.equal(uniform[0]["action"], u["action"]) for u in uniform[1:])
    assert not torch.equal(uniform[1]["value"], uniform[3]["value"])


def test_greedy_each_equals_uniform_gathered_by_set(ref):
    from runtime import kernels as K

    board, hand, combo, _ = R.tensors(ref, CPU)
    rows, which = mixed_rows(ref["n"], shift=1)
    uniform = [dict(zip(("action", "value"), K.greedy_actions(board, hand, w, combo=combo))) for w in SETS]
    want = gathered(uniform, which)
    act, val = K.greedy_actions_each(board, hand, rows, combo=combo)
    assert torch.equal(act, want["action"]) and torch.equal(val, want["value"])
    assert any(not torch.equal(uniform[0]["action"], u["action"]) for u in uniform[1:])
    # depth 1 of the plan call is the greedy call, row by row
    one = K.plan_actions_each(board, hand, rows, 1, combo=combo)
    assert torch.equal(one["action"], act) and torch.equal(one["value"], val)


def test_equal_rows_are_the_uniform_call_and_handles_equal_pos(ref):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    n = ref["n"]
    board, hand, combo, _ = R.tensors(ref, CPU)
    for w in (SETS[1], SETS[3]):
        rows = K.weight_rows(w, n=n)
        for depth in (1, 3):
            want = K.plan_actions(board, hand, w, depth, combo=combo, want_plan=True, want_leaves=True)
            got = K.plan_actions_each(board, hand, rows, depth, combo=combo, want_plan=True, want_leaves=True)
            assert all(torch.equal(got[k], want[k]) for k in KEYS), (depth, w)
        ga, gv = K.greedy_actions(board, hand, w, combo=combo)
        ea, ev = K.greedy_actions_each(board, hand, rows, combo=combo)
        assert torch.equal(ea, ga) and torch.equal(ev, gv)

    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    rows, _ = mixed_rows(n, shift=2)
    want = K.plan_actions_each(board, hand, rows, 3, combo=combo, want_plan=True, want_leaves=True)
    o = {"action": torch.full((n,), -7, dtype=torch.int32), "value": torch.full((n,), 5, dtype=torch.int64),
         "plan": torch.full((n, 3), -7, dtype=torch.int32), "leaves": torch.full((n,), -7, dtype=torch.int32)}
    env.plan_actions_each(o["action"], rows, 3, value=o["value"], plan=o["plan"], leaves=o["leaves"])
    assert all(torch.equal(o[k], want[k]) for k in KEYS)
    ga, gv = K.greedy_actions_each(board, hand, rows, combo=combo)
    ha, hv = torch.full((n,), -7, dtype=torch.int32), torch.full((n,), 5, dtype=torch.int64)
    env.greedy_actions_each(ha, rows, value=hv)
    assert torch.equal(ha, ga) and torch.equal(hv, gv)
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before), "the handle forms changed the state"
    env.close()


def test_no_legal_action_whatever_the_row_and_null_outputs(ref):
    from runtime import kernels as K

    board, hand = no_action_positions(ref)
    rows, _ = mixed_rows(8)  # each of the four sets meets both kinds of position
    for depth in (1, 2, 3):
        got = K.plan_actions_each(board, hand, rows, depth, want_plan=True, want_leaves=True)
        assert (got["action"] == 0).all() and (got["value"] == R.INT64_MIN).all()
        assert (got["plan"] == -1).all() and (got["leaves"] == 0).all()
    act, val = K.greedy_actions_each(board, hand, rows)
    assert (act == 0).all() and (val == R.INT64_MIN).all()

    # NULL optional outputs, one at a time, on the whole set: the others are what the full call wrote
    board, hand, combo, _ = R.tensors(ref, CPU)
    n = ref["n"]
    rows, _ = mixed_rows(n)
    full = K.plan_actions_each(board, hand, rows, 3, combo=combo, want_plan=True, want_leaves=True)
    for skip in ("value", "plan", "leaves"):
        got = K.plan_actions_each(board, hand, rows, 3, combo=combo, want_value=skip != "value",
                                  want_plan=skip != "plan", want_leaves=skip != "leaves")
        assert skip not in got and all(torch.equal(got[k], full[k]) for k in got), skip
    act, val = K.greedy_actions_each(board, hand, rows, combo=combo, want_value=False)
    assert val is None and torch.equal(act, K.greedy_actions_each(board, hand, rows, combo=combo)[0])
    assert torch.equal(K.plan_actions_each(board, hand, rows, 3)["action"],  # a NULL combo column reads as 0
                       K.plan_actions_each(board, hand, rows, 3, combo=torch.zeros_like(combo))["action"])


# Every refusal rule of the four entry points, in the style of tests/test_abi.py's lookahead rows: the arguments of
# an accepted call by name, overridden one at a time (None = NULL), and the text after "<entry point>: ".
_POS = dict(board=FAKE, hand=FAKE)
_GOOD = dict(pos=_POS, n=4, d_w=FAKE, depth=3, d_action=FAKE, d_value=None, out=dict(action=FAKE))
_ARGS = {"greedy_actions_each": ("d_w", "d_action", "d_value"), "plan_actions_each": ("d_w", "depth", "out")}
_NO_POS = [dict(pos=None), dict(pos=dict(board=None, hand=FAKE)), dict(pos=dict(board=FAKE, hand=None))]
_T_GREEDY = "positions (board, hand), n > 0, weight rows and d_action are required"
_T_PLAN = "positions (board, hand), n > 0, weight rows, depth in 1..3 and out->action are required"
_PLAN_ARGS = [dict(d_w=None), dict(out=None), dict(out={}), dict(depth=0), dict(depth=4)]
POS_REFUSALS = ([("greedy_actions_each", kw, _T_GREEDY)
                 for kw in _NO_POS + [dict(n=-1), dict(n=0), dict(d_w=None), dict(d_action=None)]]
                + [("plan_actions_each", kw, _T_PLAN) for kw in _NO_POS + [dict(n=-1), dict(n=0)] + _PLAN_ARGS])
ENV_REFUSALS = ([("greedy_actions_each", kw, "weight rows and d_action are required")
                 for kw in (dict(d_w=None), dict(d_action=None))]
                + [("plan_actions_each", kw, "weight rows, depth in 1..3 and out->action are required")
                   for kw in _PLAN_ARGS])


def _call(lib, family, kw, env_form=False, handle=None):
    from runtime import lib as L

    a = {**_GOOD, **kw}
    pos = L.Positions(**a["pos"]) if a["pos"] is not None else None  # alive until the call returns
    out = L.PlanOut(**a["out"]) if a["out"] is not None else None
    a["out"] = C.byref(out) if out is not None else None
    rest = [a[k] for k in _ARGS[family]] + [None]  # stream
    if env_form:
        return getattr(lib, f"bb_{family}")(handle, *rest)
    return getattr(lib, f"bb_{family}_pos")(C.byref(pos) if pos is not None else None, a["n"], *rest)


def _ids(rows):
    return [f"{i}-{fam}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for i, (fam, kw, _) in enumerate(rows)]


@pytest.mark.parametrize("family,kw,text", POS_REFUSALS, ids=_ids(POS_REFUSALS))
def test_each_pos_rules_are_one_set_for_both_backends(lib, host, family, kw, text):
    """libbbvec.so refuses before any HIP call (so this needs no GPU), the host library answers the same code, and
    bb_last_error(NULL) is the same string from both."""
    from runtime import lib as L

    for backend in (lib, host):
        assert _call(backend, family, kw) == -1  # BB_ERR_ARG
        assert L.last_error(lib=backend) == f"bb_{family}_pos: {text}"


@pytest.mark.parametrize("family,kw,text", ENV_REFUSALS, ids=_ids(ENV_REFUSALS))
def test_each_handle_rules_on_the_host_backend(host, family, kw, text):
    from runtime import lib as L
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    assert _call(host, family, kw, env_form=True, handle=env.handle) == -1  # BB_ERR_ARG
    assert L.last_error(env.handle, host) == f"bb_{family}: {text}"
    assert _call(host, family, {}, env_form=True, handle=None) == -1  # a NULL handle: a bare BB_ERR_ARG
    env.close()
