"""The argument rules of bb_board_terms(_pos) and bb_plan_actions_ext(_pos) (csrc/bb_look_rules.h, one copy for
both backends), in the style of tests/test_abi.py's lookahead rows: the arguments of an accepted call by name,
overridden one at a time (None = NULL), and the text after "<entry point>: ".  libbbvec.so refuses before any HIP
call, so none of this needs a GPU.  Also the struct's layout as the C compiler sees it, and n == 0."""
import ctypes as C
import os
import subprocess

import pytest

from runtime import lib as L

FAKE = 0x10000  # a non-NULL pointer no refused call dereferences
HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include")

_POS = dict(board=FAKE, hand=FAKE)
_GOOD = dict(pos=_POS, n=4, d_board=FAKE, d_terms=FAKE, d_w=FAKE, w_stride=1, depth=3, out=dict(action=FAKE))
_ARGS = {"board_terms": ("d_terms",), "plan_actions_ext": ("d_w", "w_stride", "depth", "out")}
_NO_POS = [dict(pos=None), dict(pos=dict(board=None, hand=FAKE)), dict(pos=dict(board=FAKE, hand=None))]
_EXT_RULES = [(dict(d_w=None), "weight rows are NULL"), (dict(w_stride=2), "w_stride must be 0 or 1"),
              (dict(w_stride=-1), "w_stride must be 0 or 1"), (dict(w_stride=12), "w_stride must be 0 or 1"),
              (dict(depth=0), "depth must be 1..3"), (dict(depth=4), "depth must be 1..3"),
              (dict(out=None), "out is NULL"), (dict(out={}), "out->action is NULL")]
POS_REFUSALS = ([("plan_actions_ext", kw, "positions (board, hand) are NULL") for kw in _NO_POS]
                + [("plan_actions_ext", dict(n=-1), "n is negative")]
                + [("plan_actions_ext", kw, text) for kw, text in _EXT_RULES]
                + [("board_terms", dict(d_board=None), "board is NULL"), ("board_terms", dict(n=-1), "n is negative"),
                   ("board_terms", dict(d_terms=None), "d_terms is NULL")])
ENV_REFUSALS = ([("plan_actions_ext", kw, text) for kw, text in _EXT_RULES]
                + [("board_terms", dict(d_terms=None), "d_terms is NULL")])


def _call(lib, family, kw, env_form=False, handle=None):
    a = {**_GOOD, **kw}
    pos = L.Positions(**a["pos"]) if a["pos"] is not None else None  # alive until the call returns
    out = L.PlanOut(**a["out"]) if a["out"] is not None else None
    a["out"] = C.byref(out) if out is not None else None
    rest = [a[k] for k in _ARGS[family]] + [None]  # stream
    if env_form:
        return getattr(lib, f"bb_{family}")(handle, *rest)
    first = a["d_board"] if family == "board_terms" else (C.byref(pos) if pos is not None else None)
    return getattr(lib, f"bb_{family}_pos")(first, a["n"], *rest)


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


@pytest.mark.parametrize("family", ["board_terms", "plan_actions_ext"])
def test_no_positions_are_accepted_and_nothing_is_read(lib, host, family):
    for backend in (lib, host):
        assert _call(backend, family, dict(n=0)) == 0  # FAKE pointers: a call that read them would crash


@pytest.mark.parametrize("family,kw,text", ENV_REFUSALS, ids=_ids(ENV_REFUSALS))
def test_handle_rules_on_the_host_backend(host, family, kw, text):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    assert _call(host, family, kw, env_form=True, handle=env.handle) == -1  # BB_ERR_ARG
    assert L.last_error(env.handle, host) == f"bb_{family}: {text}"
    assert _call(host, family, {}, env_form=True, handle=None) == -1  # a NULL handle: a bare BB_ERR_ARG
    env.close()


def test_eval_weights_layout_and_abi_version(lib, host, tmp_path):
    """bb_eval_weights as the C compiler lays it out against the ctypes mirror; the additions left the ABI at 9."""
    assert lib.bb_abi_version() == host.bb_abi_version() == L.ABI_VERSION == 9
    fields = [f"base.{k}" for k in L.GREEDY_FIELDS] + list(L.TERM_FIELDS)
    src = ['#include <stddef.h>\n#include <stdio.h>\n#include "bbvec.h"\nint main(void) {',
           'printf("%zu\\n", sizeof(bb_eval_weights));']
    src += [f'printf("%zu\\n", offsetof(bb_eval_weights, {f}));' for f in fields]
    (tmp_path / "sizes.cpp").write_text("\n".join(src) + "\nreturn 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", HEADER_DIR, str(tmp_path / "sizes.cpp"), "-o", exe],
                   check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [48] + [4 * j for j in range(12)]
    assert C.sizeof(L.EvalWeights) == 48 and L.EvalWeights.perimeter.offset == 32 and L.EvalWeights.fits.offset == 44
    for name in ("bb_board_terms_pos", "bb_board_terms", "bb_plan_actions_ext_pos", "bb_plan_actions_ext"):
        assert name in L.SIGNATURES and name in L.HOST_SYMBOLS and hasattr(lib, name) and hasattr(host, name)
