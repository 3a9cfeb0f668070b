"""The argument rules of bb_plan2_values(_pos) (csrc/bb_look_rules.h, one copy for both backends), in the style of
tests/test_values_ext_abi.py: the arguments of an accepted call by name, overridden one at a time (None = NULL), and
the text after "<entry point>: ".  libbbvec.so refuses before any HIP call, so none of this needs a GPU."""
import ctypes as C

import pytest

from runtime import lib as L

FAKE = 0x10000  # a non-NULL pointer no refused call dereferences
_GOOD = dict(pos=dict(board=FAKE, hand=FAKE), d_stream=None, n=4, d_w=FAKE, w_stride=1, depth=3, k=8, deals=16, seed=1,
             work=FAKE, work_bytes=1 << 20, out=dict(action=FAKE))
RULES = [(dict(d_w=None), "weight rows are NULL"), (dict(w_stride=2), "w_stride must be 0 or 1"),
         (dict(w_stride=-1), "w_stride must be 0 or 1"), (dict(out=None), "out is NULL"),
         (dict(out={}), "all five outputs are NULL"), (dict(depth=0), "depth must be 1..3"),
         (dict(depth=4), "depth must be 1..3"), (dict(k=0), "candidates must be 1..192"),
         (dict(k=193), "candidates must be 1..192"), (dict(deals=0), "deals must be 1..1024"),
         (dict(deals=1025), "deals must be 1..1024"), (dict(work=None), "d_work is NULL"),
         (dict(work_bytes=4 * (192 * 12 + 8 * 28 + 8 * 16 * 8) - 8), "work_bytes is below bb_plan2_work_bytes")]
POS_RULES = ([(kw, "positions (board, hand) are NULL") for kw in
              (dict(pos=None), dict(pos=dict(board=None, hand=FAKE)), dict(pos=dict(board=FAKE, hand=None)))]
             + [(dict(n=-1), "n is negative")] + RULES)


def _call(lib, kw, handle=None, env_form=False):
    a = {**_GOOD, **kw}
    pos = L.Positions(**a["pos"]) if a["pos"] is not None else None
    out = L.Plan2Out(**a["out"]) if a["out"] is not None else None
    rest = [a["d_w"], a["w_stride"], a["depth"], a["k"], a["deals"], a["seed"], a["work"], a["work_bytes"],
            C.byref(out) if out is not None else None, None]
    if env_form:
        return lib.bb_plan2_values(handle, a["d_stream"], *rest)
    return lib.bb_plan2_values_pos(C.byref(pos) if pos is not None else None, a["d_stream"], a["n"], *rest)


def _ids(rows):
    return [f"{i}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for i, (kw, _) in enumerate(rows)]


@pytest.fixture(scope="module")
def host():
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.mark.parametrize("kw,text", POS_RULES, ids=_ids(POS_RULES))
def test_pos_rules_are_one_set_for_both_backends(lib, host, kw, text):
    for backend in (lib, host):
        assert _call(backend, kw) == -1  # BB_ERR_ARG
        assert L.last_error(lib=backend) == f"bb_plan2_values_pos: {text}"


def test_no_positions_are_accepted_and_nothing_is_read(lib, host):
    for backend in (lib, host):
        assert _call(backend, dict(n=0)) == 0  # FAKE pointers: a call that read them would crash
        assert _call(backend, dict(n=0, work_bytes=0)) == 0
        assert _call(backend, dict(work_bytes=4 * (192 * 12 + 8 * 28 + 8 * 16 * 8) - 8, n=0)) == 0


@pytest.mark.parametrize("kw,text", RULES, ids=_ids(RULES))
def test_handle_rules_on_the_host_backend(host, kw, text):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    assert _call(host, kw, handle=env.handle, env_form=True) == -1
    assert L.last_error(env.handle, host) == f"bb_plan2_values: {text}"
    assert _call(host, {}, handle=None, env_form=True) == -1  # a NULL handle: a bare BB_ERR_ARG
    env.close()


def test_size_query_symbols_and_abi_version(lib, host):
    assert lib.bb_abi_version() == host.bb_abi_version() == L.ABI_VERSION == 9
    for name in ("bb_plan2_work_bytes", "bb_plan2_values_pos", "bb_plan2_values"):
        assert name in L.SIGNATURES and name in L.HOST_SYMBOLS and hasattr(lib, name) and hasattr(host, name)
    for args in ((0, 1, 1), (1, 1, 1), (4, 8, 16), (512, 8, 16), (3, 192, 1024), (-1, 1, 1), (1, 0, 1), (1, 193, 1),
                 (1, 1, 0), (1, 1, 1025)):
        assert lib.bb_plan2_work_bytes(*args) == host.bb_plan2_work_bytes(*args)
    assert lib.bb_plan2_work_bytes(4, 8, 16) == 4 * (192 * 12 + 8 * 28 + 8 * 16 * 8)
    assert lib.bb_plan2_work_bytes(-1, 1, 1) < 0
