"""The argument rules of bb_plan_values_ext(_pos) and bb_refill_values_ext(_pos) (csrc/bb_look_rules.h, one copy for
both backends), in the style of tests/test_eval_terms_abi.py: the arguments of an accepted call by name, overridden
one at a time (None = NULL), and the text after "<entry point>: ".  libbbvec.so refuses before any HIP call, so none
of this needs a GPU.  Also n == 0, and the additions left the ABI at 9."""
import ctypes as C

import pytest

from runtime import lib as L

FAKE = 0x10000  # a non-NULL pointer no refused call dereferences

_POS = dict(board=FAKE, hand=FAKE)
_GOOD = dict(pos=_POS, n=4, d_board=FAKE, d_combo=FAKE, d_stream=FAKE, d_w=FAKE, w_stride=1, depth=3, deals=8, seed=1,
             pv=dict(q=FAKE), rv=dict(value=FAKE))
_NO_POS = [dict(pos=None), dict(pos=dict(board=None, hand=FAKE)), dict(pos=dict(board=FAKE, hand=None))]
_ROW_RULES = [(dict(d_w=None), "weight rows are NULL"), (dict(w_stride=2), "w_stride must be 0 or 1"),
              (dict(w_stride=-1), "w_stride must be 0 or 1"), (dict(w_stride=12), "w_stride must be 0 or 1")]
_DEPTH = [(dict(depth=0), "depth must be 1..3"), (dict(depth=4), "depth must be 1..3")]
_PV_RULES = _ROW_RULES + [(dict(pv=None), "out is NULL"), (dict(pv={}), "all four outputs are NULL")] + _DEPTH
_RV_RULES = (_ROW_RULES + [(dict(rv=None), "out is NULL"), (dict(rv={}), "all three outputs are NULL")] + _DEPTH
             + [(dict(deals=0), "deals must be 1..1024"), (dict(deals=1025), "deals must be 1..1024")])
POS_REFUSALS = ([("plan_values_ext", kw, "positions (board, hand) are NULL") for kw in _NO_POS]
                + [("plan_values_ext", dict(n=-1), "n is negative")]
                + [("plan_values_ext", kw, text) for kw, text in _PV_RULES]
                + [("refill_values_ext", dict(d_board=None), "board is NULL"),
                   ("refill_values_ext", dict(n=-1), "n is negative")]
                + [("refill_values_ext", kw, text) for kw, text in _RV_RULES])
ENV_REFUSALS = ([("plan_values_ext", kw, text) for kw, text in _PV_RULES]
                + [("refill_values_ext", kw, text) for kw, text in _RV_RULES])


def _call(lib, family, kw, env_form=False, handle=None):
    a = {**_GOOD, **kw}
    pos = L.Positions(**a["pos"]) if a["pos"] is not None else None  # alive until the call returns
    if family == "plan_values_ext":
        out = L.PlanValuesOut(**a["pv"]) if a["pv"] is not None else None
        o = C.byref(out) if out is not None else None
        rest = [a["d_w"], a["w_stride"], a["depth"], o, None]
        if env_form:
            return lib.bb_plan_values_ext(handle, *rest)
        return lib.bb_plan_values_ext_pos(C.byref(pos) if pos is not None else None, a["n"], *rest)
    out = L.RefillValuesOut(**a["rv"]) if a["rv"] is not None else None
    o = C.byref(out) if out is not None else None
    rest = [a["d_w"], a["w_stride"], a["depth"], a["deals"], a["seed"], o, None]
    if env_form:
        return lib.bb_refill_values_ext(handle, a["d_stream"], *rest)
    return lib.bb_refill_values_ext_pos(a["d_board"], a["d_combo"], a["d_stream"], a["n"], *rest)


def _ids(rows):
    return [f"{i}-{fam}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for i, (fam, kw, _) in enumerate(rows)]


@pytest.fixture(scope="module")
def host():
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.mark.parametrize("family,kw,text", POS_REFUSALS, ids=_ids(POS_REFUSALS))
def test_pos_rules_are_one_set_for_both_backends(lib, host, family, kw, text):
    for backend in (lib, host):
        assert _call(backend, family, kw) == -1  # BB_ERR_ARG
        assert L.last_error(lib=backend) == f"bb_{family}_pos: {text}"


@pytest.mark.parametrize("family", ["plan_values_ext", "refill_values_ext"])
def test_no_positions_are_accepted_and_nothing_is_read(lib, host, family):
    for backend in (lib, host):
        assert _call(backend, family, dict(n=0)) == 0  # FAKE pointers: a call that read them would crash
        assert _call(backend, family, dict(n=0, w_stride=0)) == 0


@pytest.mark.parametrize("family,kw,text", ENV_REFUSALS, ids=_ids(ENV_REFUSALS))
def test_handle_rules_on_the_host_backend(host, family, kw, text):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    assert _call(host, family, kw, env_form=True, handle=env.handle) == -1  # BB_ERR_ARG
    assert L.last_error(env.handle, host) == f"bb_{family}: {text}"
    assert _call(host, family, {}, env_form=True, handle=None) == -1  # a NULL handle: a bare BB_ERR_ARG
    env.close()


def test_the_rules_are_the_parents_with_weight_rows_for_weights(lib):
    """The eight-weight entry points name the same rules in the same order, "weights" where these say "weight rows"."""
    w = L.greedy_weights({})
    pos, pv, rv = L.Positions(**_POS), L.PlanValuesOut(), L.RefillValuesOut()
    assert lib.bb_plan_values_pos(C.byref(pos), 4, None, 3, C.byref(pv), None) == -1
    assert L.last_error(lib=lib) == "bb_plan_values_pos: weights are NULL"
    assert lib.bb_plan_values_pos(C.byref(pos), 4, C.byref(w), 3, C.byref(pv), None) == -1
    assert L.last_error(lib=lib) == "bb_plan_values_pos: all four outputs are NULL"
    assert lib.bb_refill_values_pos(FAKE, None, None, 4, C.byref(w), 3, 8, 1, C.byref(rv), None) == -1
    assert L.last_error(lib=lib) == "bb_refill_values_pos: all three outputs are NULL"


def test_symbols_and_abi_version(lib, host):
    assert lib.bb_abi_version() == host.bb_abi_version() == L.ABI_VERSION == 9
    for name in ("bb_plan_values_ext_pos", "bb_plan_values_ext", "bb_refill_values_ext_pos", "bb_refill_values_ext"):
        assert name in L.SIGNATURES and name in L.HOST_SYMBOLS and hasattr(lib, name) and hasattr(host, name)
