"""The C-ABI library loads (no GPU needed) and exports every symbol that
include/bbvec.h declares; host-only entry points are exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from runtime import lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "bbvec.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bb_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    assert set(declared_symbols()) == set(L.SIGNATURES)


def test_library_exports_every_symbol(lib):
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert lib.bb_abi_version() == L.ABI_VERSION == 9


def test_build_id_is_these_sources(lib):
    """bb_build_id ties the binary to HEAD's sources: the id is the hash of csrc/, include/bbvec.h and the
    flags, the .so carries it where build.py reads it without loading, and load() refuses a mismatch."""
    from runtime import build as B

    sid = B.source_id()
    assert len(sid) == 16 and lib.bb_build_id().decode() == sid == B.built_id(L.LIB_PATH)
    assert L.build_id() == sid
    host = B.build_host_lib(verbose=False)
    assert B.built_id(host) == B.host_source_id() == L.build_id(host=True)


def _quoted_includes(sources):
    """Every file reached from `sources` through #include "..." lines, followed recursively."""
    seen, todo = set(), [os.path.realpath(s) for s in sources]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), flags=re.M):
            todo.append(os.path.realpath(os.path.join(os.path.dirname(f), inc)))
    return seen


def test_build_id_hashes_every_included_file():
    """A header that a source includes but the id does not hash would leave a stale library looking current."""
    from runtime import build as B

    for sources, headers in ((B.SOURCES, B.HEADERS), (B.HOST_SOURCES, B.HOST_HEADERS)):
        hashed = {os.path.realpath(os.path.join(B.CSRC, f)) for f in sources + headers} | {os.path.realpath(B.HEADER)}
        found = _quoted_includes([os.path.join(B.CSRC, s) for s in sources])
        assert len(found) > len(sources)
        assert found <= hashed, sorted(os.path.relpath(f, B.CSRC) for f in found - hashed)


def test_stale_library_is_refused(lib, tmp_path, monkeypatch):
    """A library whose id differs from the sources beside it is refused by name, not loaded silently."""
    from runtime import build as B

    monkeypatch.setattr(B, "source_id", lambda: "0" * 16)
    monkeypatch.setattr(L, "_lib", None)
    with pytest.raises(L.BBNativeError, match="built from other sources"):
        L.load()


ARG_STRUCTS = {"bb_bn_fwd": L.BnFwd, "bb_wgrad_reduce": L.WgradReduce, "bb_bn_bwd": L.BnBwd,
               "bb_ppo_loss_args": L.PpoLossArgs}


def test_struct_sizes(lib, tmp_path):
    """The argument structs as the C compiler lays them out against the ctypes mirrors: the size, and every
    field's name and offset (a transposed pointer / int32 pair moves an offset)."""
    assert L.INFO_BYTES == 56
    src = ["#include <stddef.h>\n#include <stdio.h>\n#include \"bbvec.h\"\nint main(void) {"]
    want = []
    for cname, cls in ARG_STRUCTS.items():
        src.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for field, _ in cls._fields_:
            src.append(f'printf("%zu\\n", offsetof({cname}, {field}));')
            want.append(getattr(cls, field).offset)
    (tmp_path / "sizes.cpp").write_text("\n".join(src) + "\nreturn 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.dirname(HEADER),  # the host library's compiler
                    str(tmp_path / "sizes.cpp"), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


FAKE = 0x10000  # a host integer standing for a 16-byte aligned device pointer: validation never dereferences it


def _bn_fwd(**kw):
    a = dict(x=FAKE, dtype=1, nhwc=1, N=2, C=64, HW=64, weight=FAKE, bias=FAKE, eps=1e-5, relu=1, ws=FAKE,
             save_mean=FAKE, save_invstd=FAKE, y=FAKE)
    return L.BnFwd(**{**a, **kw})


def _bn_bwd(**kw):
    a = dict(x=FAKE, dy=FAKE, dtype=1, nhwc=1, N=2, C=64, HW=64, weight=FAKE, bias=FAKE, save_mean=FAKE,
             save_invstd=FAKE, relu=0, ws=FAKE, dx=FAKE)
    return L.BnBwd(**{**a, **kw})


def _loss(**kw):
    a = {k: FAKE for k, _ in L.PpoLossArgs._fields_ if k not in ("bf16", "B", "clip", "value_coef", "entropy_coef")}
    return L.PpoLossArgs(**{**a, "B": 4, "clip": 0.2, "value_coef": 0.5, "entropy_coef": 0.01, **kw})


_RED =dict(ws=FAKE, chunks=4, cin=64, cout=128, w_layout=0, dw=FAKE)
_SHAPE = [(dict(dtype=2), "dtype"), (dict(nhwc=2), "layout"), (dict(N=0), "empty"),
          (dict(nhwc=0, HW=4), "16-byte"),  # NCHW bf16 rows of 8 bytes
          (dict(C=24), "power of two")]     # NHWC bf16 rows of 48 bytes
BAD_ARGS = (
    [("bb_bn_forward", None, "NULL")]
    + [("bb_bn_forward", _bn_fwd(**kw), msg) for kw, msg in _SHAPE]
    + [("bb_bn_forward", _bn_fwd(**{k: None}), "NULL argument")
       for k in ("x", "weight", "bias", "ws", "save_mean", "save_invstd", "y")]
    + [("bb_bn_forward", _bn_fwd(ws=FAKE + 8), "ws must be 16-byte aligned"),
       ("bb_bn_forward", _bn_fwd(res=FAKE + 8), "res must be 16-byte aligned"),
       ("bb_bn_forward", _bn_fwd(part=FAKE, nb_part=0), "nb_part"),
       ("bb_bn_backward", None, "NULL")]
    + [("bb_bn_backward", _bn_bwd(**kw), msg) for kw, msg in _SHAPE]
    + [("bb_bn_backward", _bn_bwd(**{k: None}), "NULL argument")
       for k in ("x", "dy", "weight", "bias", "save_mean", "save_invstd", "ws", "dx")]
    + [("bb_bn_backward", _bn_bwd(ws=FAKE + 8), "ws must be 16-byte aligned"),
       ("bb_bn_backward", _bn_bwd(part=FAKE, nb_part=0), "nb_part"),
       ("bb_bn_backward", _bn_bwd(y=FAKE), "y and gres"),
       ("bb_bn_backward", _bn_bwd(gres=FAKE), "y and gres"),
       ("bb_bn_backward", _bn_bwd(y=FAKE, gres=FAKE, part=FAKE, nb_part=2), "no part"),
       ("bb_bn_backward", _bn_bwd(y=FAKE, gres=FAKE, relu=1), "relu = 0")]
    + [("bb_bn_backward", _bn_bwd(reduce=L.WgradReduce(**{**_RED, **kw})), "convolution reduction")
       for kw in (dict(cin=3), dict(cout=96), dict(dw=None), dict(chunks=0), dict(w_layout=2))]
    + [(fn, None, "bad arguments") for fn in ("bb_ppo_loss_forward", "bb_ppo_loss_backward", "bb_ppo_loss_fused")]
    + [(fn, _loss(B=0), "bad arguments") for fn in ("bb_ppo_loss_forward", "bb_ppo_loss_backward", "bb_ppo_loss_fused")]
    + [(fn, _loss(**{k: None}), "bad arguments")
       for fn, ks in (("bb_ppo_loss_forward", "logits values mask actions old_logp adv ret ws cnt stats"),
                      ("bb_ppo_loss_backward", "logits values mask actions old_logp adv ret grad_loss dlogits dvalues"),
                      ("bb_ppo_loss_fused", "logits values mask actions old_logp adv ret grad_loss dlogits dvalues "
                                            "ws cnt stats"))
       for k in ks.split()])


@pytest.mark.parametrize("fn,args,msg", BAD_ARGS, ids=[f"{i}-{c[0]}-{c[2]}" for i, c in enumerate(BAD_ARGS)])
def test_argument_structs_are_validated_before_any_hip_call(lib, fn, args, msg):
    """Every rule of bb_bn_fwd / bb_bn_bwd / bb_wgrad_reduce / bb_ppo_loss_args is checked before the first HIP
    call, so it shows without a GPU: BB_ERR_ARG, and bb_last_error(NULL) names the rule."""
    assert getattr(lib, fn)(C.byref(args) if args is not None else None, None) == -1  # BB_ERR_ARG
    assert msg in L.last_error()


# The lookahead entry points: the arguments of an accepted call by name (None = NULL; pos / out name the fields of
# their struct), the order they are passed in, and every refusal rule as (entry point, overrides, the text after
# "<entry point>: ").  The rules live in csrc/bb_look_rules.h, which both libraries include.
_POS = dict(board=FAKE, hand=FAKE)
_LOOK_GOOD = dict(pos=_POS, n=4, cfg=True, w=True, depth=3, d_action=FAKE, d_value=None)
_LOOK_OUT = {"afterstates": (L.AfterstateOut, dict(board=FAKE)), "greedy_actions": (None, None),
             "plan_actions": (L.PlanOut, dict(action=FAKE)), "plan_values": (L.PlanValuesOut, dict(safe=FAKE))}
_LOOK_ARGS = {"afterstates": ("cfg", "out"), "greedy_actions": ("w", "d_action", "d_value"),
              "plan_actions": ("w", "depth", "out"), "plan_values": ("w", "depth", "out")}
_NO_POS = [dict(pos=None), dict(pos=dict(board=None, hand=FAKE)), dict(pos=dict(board=FAKE, hand=None))]
_T_AFTER = "positions (board, hand), n > 0, cfg and out are required"
_T_GREEDY = "positions (board, hand), n > 0, weights and d_action are required"
_T_PLAN = "positions (board, hand), n > 0, weights, depth in 1..3 and out->action are required"
_VALUES_RULES = [(dict(w=None), "weights are NULL"), (dict(out=None), "out is NULL"),
                 (dict(out={}), "all four outputs are NULL"), (dict(depth=0), "depth must be 1..3"),
                 (dict(depth=4), "depth must be 1..3")]
LOOK_POS_REFUSALS = (
    [("afterstates", kw, _T_AFTER) for kw in _NO_POS + [dict(n=-1), dict(n=0), dict(cfg=None), dict(out=None)]]
    + [("greedy_actions", kw, _T_GREEDY) for kw in _NO_POS + [dict(n=-1), dict(n=0), dict(w=None), dict(d_action=None)]]
    + [("plan_actions", kw, _T_PLAN) for kw in _NO_POS + [dict(n=-1), dict(n=0), dict(w=None), dict(out=None),
                                                          dict(out={}), dict(depth=0), dict(depth=4)]]
    + [("plan_values", kw, "positions (board, hand) are NULL") for kw in _NO_POS]
    + [("plan_values", dict(n=-1), "n is negative")] + [("plan_values", kw, msg) for kw, msg in _VALUES_RULES])
_T_PLAN_ENV = "weights, depth in 1..3 and out->action are required"
LOOK_ENV_REFUSALS = (
    [("afterstates", dict(out=None), "out is NULL")]
    + [("greedy_actions", kw, "weights and d_action are required") for kw in (dict(w=None), dict(d_action=None))]
    + [("plan_actions", kw, _T_PLAN_ENV) for kw in (dict(w=None), dict(out=None), dict(out={}), dict(depth=0),
                                                    dict(depth=4))]
    + [("plan_values", kw, msg) for kw, msg in _VALUES_RULES])


def _look_call(lib, family, kw, env_form=False, handle=None):
    """Call bb_<family>_pos, or bb_<family> with a handle, with the accepted arguments overridden by kw."""
    from runtime.device_env import DEFAULT_REWARDS

    cls, fields = _LOOK_OUT[family]
    a = {**_LOOK_GOOD, "out": fields, **kw}
    keep = {"pos": L.Positions(**a["pos"]) if a["pos"] is not None else None,  # alive until the call returns
            "cfg": L.reward_cfg(DEFAULT_REWARDS) if a["cfg"] else None,
            "w": L.greedy_weights({"lines": 1}) if a["w"] else None,
            "out": cls(**a["out"]) if cls is not None and a["out"] is not None else None}
    ref = {k: C.byref(v) if v is not None else None for k, v in keep.items()}
    names = [k for k in _LOOK_ARGS[family] if not (env_form and k == "cfg")]  # a handle carries its reward config
    rest = [ref[k] if k in ref else a[k] for k in names] + [None]  # stream
    if env_form:
        return getattr(lib, f"bb_{family}")(handle, *rest)
    return getattr(lib, f"bb_{family}_pos")(ref["pos"], a["n"], *rest)


def _look_ids(rows):
    return [f"{i}-{fam}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for i, (fam, kw, _) in enumerate(rows)]


@pytest.mark.parametrize("family,kw,text", LOOK_POS_REFUSALS, ids=_look_ids(LOOK_POS_REFUSALS))
def test_lookahead_pos_rules_are_one_set_for_both_backends(lib, family, kw, text):
    """Every refusal rule of the four stateless lookahead entry points: libbbvec.so answers BB_ERR_ARG before any
    HIP call (so this passes without a GPU), the host library answers the same code, and bb_last_error(NULL) is
    the same string from both."""
    want = f"bb_{family}_pos: {text}"
    for backend in (lib, L.load_host()):
        assert _look_call(backend, family, kw) == -1  # BB_ERR_ARG
        assert L.last_error(lib=backend) == want


def test_plan_values_pos_alone_accepts_no_positions(lib):
    """The asymmetry bb_look_rules.h records: n == 0 is refused by three of the _pos forms (rows above) and accepted
    by bb_plan_values_pos, which then does nothing (no HIP call either)."""
    for backend in (lib, L.load_host()):
        assert _look_call(backend, "plan_values", dict(n=0)) == 0


@pytest.fixture(scope="module")
def host_env():
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    yield env
    env.close()


@pytest.mark.parametrize("family,kw,text", LOOK_ENV_REFUSALS, ids=_look_ids(LOOK_ENV_REFUSALS))
def test_lookahead_handle_rules_on_the_host_backend(host_env, family, kw, text):
    """The handle forms' rules, from the same header, on a host env: BB_ERR_ARG with the rule as the handle's error;
    a NULL handle is a bare BB_ERR_ARG.  (On libbbvec.so a handle needs a device: the GPU tests cover it.)"""
    host = L.load_host()
    assert _look_call(host, family, kw, env_form=True, handle=host_env.handle) == -1  # BB_ERR_ARG
    assert L.last_error(host_env.handle, host) == f"bb_{family}: {text}"
    assert _look_call(host, family, {}, env_form=True, handle=None) == -1


@pytest.mark.parametrize("seed", [0, 1, 42, 43, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7, 2 ** 63, 2 ** 64 - 1])
def test_pcg64_seeding_matches_numpy(lib, seed):
    w = L.pcg64_seed(seed)
    st = np.random.PCG64(seed).state["state"]
    assert (w[0] << 64 | w[1]) == st["state"]
    assert (w[2] << 64 | w[3]) == st["inc"]


def test_seed42_golden_state(lib):
    import json
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_seed42.json")))
    w = L.pcg64_seed(42)
    assert str(w[0] << 64 | w[1]) == g["numpy_pcg64_seed42"]["state"]
    assert str(w[2] << 64 | w[3]) == g["numpy_pcg64_seed42"]["inc"]


def test_create_without_gpu_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctypes as C
    h = C.c_void_p()
    rc = lib.bb_create(4, 0, C.byref(L.reward_cfg(dict(
        line_clear_base=1.0, block_placed=0.01, game_over_penalty=-1.0, hole_penalty=-0.05, center_bonus=0.02,
        combo_multiplier_bonus=0.5, survival_bonus=0.001))), 1, C.byref(h))
    assert rc != 0 and "no HIP device" in L.last_error()
