"""The hand-safe mask call on the host backend (bb_safe_mask / bb_safe_mask_pos of libbbvec_host.so), on the CPU (no
GPU involved), against the references of tests/_safe_positions.py, which call neither: both modes and both forms on
the 92-position set, the crowded set, mode 1 from mode 0, bb_plan_values' safe words at depth 2 and 3, guard words
around the output, argument errors (the same text from both libraries), a finished game, and the Python surface.

The training-side checks (DeviceRollout(safe_mask=True), train() with training.safe_mask) are in
tests/test_gpu_safe_rollout.py: the PPO agent's sampler, GAE and minibatch gather are HIP-only (no CPU fallback), so
neither runs on the host backend.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _safe_positions as S

CPU = torch.device("cpu")
ERR_ARG = -1


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


def _pos_call(board, hand, mode):
    from runtime import kernels as K

    b, h = S.tensors(board, hand, CPU)
    return K.safe_mask(b, h, mode)


def test_references_are_not_vacuous(host):
    a, b = S.reference_a(), S.reference_b()
    for r in (a, b):
        assert (r["mode1"] != r["safe"]).any() and (r["safe"] != r["legal"]).any()


@pytest.mark.parametrize("mode", [0, 1])
def test_host_equals_reference_a_both_forms(host, mode):
    from runtime.device_env import DeviceEnvBatch

    ref, a = R.reference(), S.reference_a()
    want = a["mode1"] if mode else a["safe"]
    S.assert_words(_pos_call(a["board"], a["hand"], mode), want, f"_pos mode {mode}")
    env = DeviceEnvBatch(ref["n"], list(range(ref["n"])), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    out = torch.full((ref["n"], 3), -7, dtype=torch.int64)
    got = env.sampling_mask(out) if mode else env.safe_mask(out, depth=2)
    assert got is out
    S.assert_words(out, want, f"handle mode {mode}")
    if not mode:
        S.assert_words(env.safe_mask(torch.zeros_like(out), depth=3), want, "handle depth 3")
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_host_equals_reference_b(host, mode):
    b = S.reference_b()
    S.assert_words(_pos_call(b["board"], b["hand"], mode), b["mode1"] if mode else b["safe"], f"crowded mode {mode}")


@pytest.mark.parametrize("which", ["a", "b"])
def test_mode1_is_safe_else_legal_row_by_row(host, which):
    r = S.reference_a() if which == "a" else S.reference_b()
    safe = S.as_u64(_pos_call(r["board"], r["hand"], 0))
    got = S.as_u64(_pos_call(r["board"], r["hand"], 1))
    S.assert_words(got, S.sampling(safe, r["legal"]), "mode 1 from mode 0")
    fallback = (safe == 0).all(axis=1) & (r["legal"] != 0).any(axis=1)
    assert fallback.sum() >= (1 if which == "a" else 20)
    assert (got[fallback] == r["legal"][fallback]).all() and not (got & ~r["legal"]).any()


@pytest.mark.parametrize("depth", [2, 3])
def test_mode0_equals_plan_values_safe(host, depth):
    from runtime import kernels as K

    for r in (S.reference_a(), S.reference_b()):
        b, h = S.tensors(r["board"], r["hand"], CPU)
        want = K.plan_values(b, h, {}, depth, want=("safe",))["safe"]
        assert torch.equal(K.safe_mask(b, h, 0), want), depth


def test_nothing_written_beyond_the_output(host):
    from runtime import lib as L

    b = S.reference_b()
    n = len(b["board"])
    for mode in (0, 1):
        buf = np.full(3 * n + 16, 0xA5A5A5A5A5A5A5A5, np.uint64)
        pos = L.Positions(board=b["board"].ctypes.data, hand=b["hand"].ctypes.data)
        assert host.bb_safe_mask_pos(C.byref(pos), n, mode, buf[8:].ctypes.data, None) == 0
        assert (buf[:8] == 0xA5A5A5A5A5A5A5A5).all() and (buf[8 + 3 * n:] == 0xA5A5A5A5A5A5A5A5).all()
        S.assert_words(buf[8:8 + 3 * n].reshape(n, 3), b["mode1"] if mode else b["safe"], f"guarded mode {mode}")


FAKE = 0x1000
_NO_POS = [None, dict(board=None, hand=FAKE), dict(board=FAKE, hand=None)]
POS_REFUSALS = ([(dict(pos=p), "positions (board, hand) are NULL") for p in _NO_POS]
                + [(dict(n=-1), "n is negative"), (dict(d_mask=None), "d_mask is NULL"),
                   (dict(mode=-1), "mode must be 0..1"), (dict(mode=2), "mode must be 0..1")])


@pytest.mark.parametrize("kw,text", POS_REFUSALS, ids=[str(i) for i in range(len(POS_REFUSALS))])
def test_pos_rules_are_one_set_for_both_backends(lib, host, kw, text):
    """Refused with BB_ERR_ARG before any HIP call (so libbbvec.so answers without a GPU), the same text from both."""
    from runtime import lib as L

    a = {"pos": dict(board=FAKE, hand=FAKE), "n": 4, "mode": 0, "d_mask": FAKE, **kw}
    pos = L.Positions(**a["pos"]) if a["pos"] is not None else None
    for backend in (lib, host):
        rc = backend.bb_safe_mask_pos(C.byref(pos) if pos is not None else None, a["n"], a["mode"], a["d_mask"], None)
        assert rc == ERR_ARG
        assert L.last_error(lib=backend) == f"bb_safe_mask_pos: {text}"


def test_no_positions_is_accepted_and_does_nothing(lib, host):
    from runtime import lib as L

    pos = L.Positions(board=FAKE, hand=FAKE)
    for backend in (lib, host):
        for mode in (0, 1):
            assert backend.bb_safe_mask_pos(C.byref(pos), 0, mode, FAKE, None) == 0


def test_handle_rules_on_the_host_backend(host):
    from runtime import lib as L
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    env.reset()
    out = np.zeros((4, 3), np.uint64)
    for args, text in (((0, None), "d_mask is NULL"), ((2, out.ctypes.data), "mode must be 0..1"),
                       ((-1, out.ctypes.data), "mode must be 0..1")):
        assert host.bb_safe_mask(env.handle, *args, None) == ERR_ARG
        assert L.last_error(env.handle, host) == f"bb_safe_mask: {text}"
    assert host.bb_safe_mask(None, 0, out.ctypes.data, None) == ERR_ARG
    assert host.bb_safe_mask(env.handle, 1, out.ctypes.data, None) == 0
    assert (out != 0).any()
    env.close()


def test_finished_game_is_all_zeros(host):
    """The game-over bit set: nothing is legal, so nothing is safe and there is nothing to fall back to; through the
    handle too, on games played to their end without auto-reset."""
    from runtime.device_env import DeviceEnvBatch

    ref = R.reference()
    i = ref["names"]["game_over"]
    for mode in (0, 1):
        assert (S.as_u64(_pos_call(ref["board"][i:i + 1], ref["hand"][i:i + 1], mode)) == 0).all()
    n = 8
    env = DeviceEnvBatch(n, list(range(50, 50 + n)), autoreset=False, device="cpu")
    env.reset()
    mb, act = torch.zeros((n, 3), dtype=torch.int64), torch.zeros(n, dtype=torch.int32)
    over = torch.zeros(n, dtype=torch.bool)
    for t in range(400):
        env.obs(mask_bits=mb)
        env.random_actions(mb, act, step=t)
        env.step(act)
        over |= env.terminated.bool()
        if over.all():
            break
    assert over.all()
    assert (((torch.from_numpy(env.state()["hand"].astype(np.int64)) >> 21) & 1) == 1).all()
    for mode in (0, 1):
        assert (env._safe_mask(mode, torch.full((n, 3), -7, dtype=torch.int64)) == 0).all()
    env.close()


def test_python_surface_checks_its_output(host):
    from runtime import kernels as K
    from runtime import lib as L

    a = S.reference_a()
    b, h = S.tensors(a["board"][:5], a["hand"][:5], CPU)
    out = torch.zeros((5, 3), dtype=torch.int64)
    assert K.safe_mask(b, h, K.SAFE_OR_LEGAL, out=out) is out
    S.assert_words(out, a["mode1"][:5], "out=")
    for bad in (torch.zeros((5, 3), dtype=torch.int32), torch.zeros((4, 3), dtype=torch.int64)):
        with pytest.raises(L.BBNativeError):
            K.safe_mask(b, h, 0, out=bad)
    with pytest.raises(L.BBNativeError, match="mode must be 0..1"):
        K.safe_mask(b, h, 2)


def test_gym_surfaces_keep_their_safe_action_mask(host):
    """VectorizedBlockBlastEnv.safe_action_mask goes through DeviceEnvBatch.safe_mask, now the new call."""
    from environment.wrappers import VectorizedBlockBlastEnv
    from runtime import kernels as K

    env = VectorizedBlockBlastEnv(6, seed=11, device="cpu")
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(7):
        got = env.safe_action_mask()
        want = K.mask_bits_to_bool(env.dev.plan_values({}, 3, out=None)["safe"]).numpy()
        assert np.array_equal(np.asarray(got, bool), want)
        legal = env.get_action_masks()
        assert not (want & ~legal).any()
        env.step(np.array([rng.choice(np.nonzero(m)[0]) if m.any() else 0 for m in legal]))
    env.close()
