"""The refill census on the host backend (bb_refill_census / bb_refill_census_pos of libbbvec_host.so), on the CPU (no
GPU involved), against tests/_census_ref.py's oracle census, which calls neither: count and every word on the
reference set, the words' symmetry, count = popcount sum, the handle form, n == 0 and a NULL output, every refusal
(the same text from both libraries), the Python argument rules, refill_hazard against exact fractions and the gym
surfaces.
"""
import ctypes as C
import fractions
import itertools

import numpy as np
import pytest
import torch

import _census_ref as CR

ERR_ARG = -1
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def got(host):
    from runtime import kernels as K

    return K.refill_census(CR.board_tensor(CR.reference()["board"]), want=("count", "solvable"))


def test_host_equals_the_oracle_on_the_reference_set(got):
    ref = CR.reference()
    assert got["count"].dtype == torch.int32 and got["solvable"].shape == (len(ref["board"]), 37, 37)
    assert got["count"].tolist() == ref["count"].tolist()
    bad = np.argwhere(CR.as_u64(got["solvable"]) != ref["solvable"])
    assert bad.size == 0, bad[:4].tolist()


def test_words_are_symmetric_and_count_is_their_popcount(got):
    w = CR.as_u64(got["solvable"])
    assert not (w >> np.uint64(37)).any()
    bits = ((w[..., None] >> np.arange(37, dtype=np.uint64)) & np.uint64(1)).astype(bool)  # [n, a, b, c]
    for perm in itertools.permutations((1, 2, 3)):
        assert np.array_equal(bits, bits.transpose(0, *perm)), perm
    assert bits.sum(axis=(1, 2, 3)).tolist() == got["count"].tolist()


def test_handle_form_equals_pos_form_and_changes_nothing(host, got):
    from runtime.device_env import DeviceEnvBatch

    ref = CR.reference()
    n = len(ref["board"])
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    env.set_state(board=ref["board"])
    before = env.state()
    count, words = torch.full((n,), -7, dtype=torch.int32), torch.full((n, 37, 37), -7, dtype=torch.int64)
    out = env.refill_census(count=count, solvable=words)
    assert out["count"] is count and out["solvable"] is words
    assert torch.equal(count, got["count"]) and torch.equal(words, got["solvable"])
    assert torch.equal(env.refill_census()["count"], got["count"])  # a fresh count
    after = env.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    env.close()


def test_each_output_alone_and_nothing_beyond_it(host):
    from runtime import lib as L

    ref = CR.reference()
    n = len(ref["board"])
    count = np.full(n + 16, -7, np.int32)
    words = np.full(n * 37 * 37 + 16, GUARD, np.uint64)
    for want_c, want_w in ((True, False), (False, True), (True, True)):
        count[:] = -7
        words[:] = GUARD
        o = L.CensusOut(count=count[8:].ctypes.data if want_c else None,
                        solvable=words[8:].ctypes.data if want_w else None)
        assert host.bb_refill_census_pos(ref["board"].ctypes.data, n, C.byref(o), None) == 0
        assert (count[:8] == -7).all() and (count[8 + n:] == -7).all()
        assert (words[:8] == GUARD).all() and (words[8 + n * 1369:] == GUARD).all()
        assert count[8:8 + n].tolist() == (ref["count"].tolist() if want_c else [-7] * n)
        if want_w:
            assert np.array_equal(words[8:8 + n * 1369].reshape(n, 37, 37), ref["solvable"])
        else:
            assert (words == GUARD).all()


FAKE = 0x1000
POS_REFUSALS = [(dict(board=None), "board is NULL"), (dict(n=-1), "n is negative"), (dict(out=None), "out is NULL"),
                (dict(out={}), "both outputs are NULL")]


@pytest.mark.parametrize("kw,text", POS_REFUSALS, ids=[t for _, t in POS_REFUSALS])
def test_pos_rules_are_one_set_for_both_backends(lib, host, kw, text):
    """Refused with BB_ERR_ARG before any HIP call (so libbbvec.so answers without a GPU), the same text from both."""
    from runtime import lib as L

    a = {"board": FAKE, "n": 4, "out": dict(count=FAKE), **kw}
    o = L.CensusOut(**a["out"]) if a["out"] is not None else None
    for backend in (lib, host):
        rc = backend.bb_refill_census_pos(a["board"], a["n"], C.byref(o) if o is not None else None, None)
        assert rc == ERR_ARG
        assert L.last_error(lib=backend) == f"bb_refill_census_pos: {text}"


def test_no_boards_is_accepted_and_does_nothing(lib, host):
    from runtime import kernels as K
    from runtime import lib as L

    for backend in (lib, host):
        for o in (L.CensusOut(count=FAKE), L.CensusOut(solvable=FAKE), L.CensusOut(count=FAKE, solvable=FAKE)):
            assert backend.bb_refill_census_pos(FAKE, 0, C.byref(o), None) == 0
    out = K.refill_census(torch.zeros(0, dtype=torch.int64), want=("count", "solvable"))
    assert out["count"].shape == (0,) and out["solvable"].shape == (0, 37, 37)


def test_handle_rules_on_the_host_backend(host):
    from runtime import lib as L
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(4, [1, 2, 3, 4], autoreset=False, device="cpu")
    env.reset()
    count = np.zeros(4, np.int32)
    for o, text in ((None, "out is NULL"), (L.CensusOut(), "both outputs are NULL")):
        assert host.bb_refill_census(env.handle, C.byref(o) if o is not None else None, None) == ERR_ARG
        assert L.last_error(env.handle, host) == f"bb_refill_census: {text}"
    o = L.CensusOut(count=count.ctypes.data)
    assert host.bb_refill_census(None, C.byref(o), None) == ERR_ARG
    assert host.bb_refill_census(env.handle, C.byref(o), None) == 0
    assert count.tolist() == [CR.NUM_HANDS] * 4  # empty boards after the reset
    env.close()


def test_python_argument_rules(host):
    from runtime import kernels as K
    from runtime import lib as L

    b = CR.board_tensor(CR.reference()["board"][:5])
    for bad in (b.to(torch.int32), b.reshape(5, 1), torch.stack([b, b], dim=1)[:, 0], b.numpy()):
        with pytest.raises(L.BBNativeError, match="board must be a contiguous torch.int64 tensor of shape"):
            K.refill_census(bad)
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.refill_census(b, want=("count", "hands"))
    with pytest.raises(L.BBNativeError, match="unknown outputs"):
        K.refill_census(b, out={"hands": torch.zeros(5, dtype=torch.int32)})
    with pytest.raises(L.BBNativeError, match="at least one of count, solvable"):
        K.refill_census(b, out={})
    for k, t in (("count", torch.zeros(5, dtype=torch.int64)), ("count", torch.zeros(4, dtype=torch.int32)),
                 ("count", torch.zeros(10, dtype=torch.int32)[::2]),
                 ("solvable", torch.zeros((5, 37, 37), dtype=torch.int32)),
                 ("solvable", torch.zeros((5, 37, 36), dtype=torch.int64))):
        with pytest.raises(L.BBNativeError, match=f"{k} must be a contiguous"):
            K.refill_census(b, out={k: t})
    out = {"count": torch.zeros(5, dtype=torch.int32)}
    assert K.refill_census(b, out=out) is out and out["count"].tolist() == CR.reference()["count"][:5].tolist()
    assert set(K.refill_census(b)) == {"count"}


@pytest.mark.parametrize("attempts", [100, 1, 7])
def test_refill_hazard_against_exact_fractions(attempts):
    from runtime import kernels as K

    counts = [0, 1, 125, 2995, 3997, 25000, 50652, 50653]
    got = K.refill_hazard(torch.tensor(counts), attempts)
    assert got.dtype == torch.float64
    for c, g in zip(counts, got.tolist()):
        want = float(fractions.Fraction(50653 - c, 50653) ** attempts)
        print(c, g, want)
        assert abs(g - want) <= 1e-12 * want, (c, g, want)
    assert got[0].item() == 1.0 and got[-1].item() == 0.0
    if attempts == 100:
        assert got.tolist() == K.refill_hazard(torch.tensor(counts)).tolist()
        assert K.refill_hazard(np.array(counts, np.int32)).tolist() == got.tolist()


def test_gym_surfaces_against_the_oracle(host):
    from environment.block_blast_env import BlockBlastEnv
    from environment.wrappers import VectorizedBlockBlastEnv
    from runtime import kernels as K

    env = VectorizedBlockBlastEnv(6, seed=11, device="cpu")
    env.reset()
    rng = np.random.default_rng(0)
    for t in range(24):
        legal = env.get_action_masks()
        env.step(np.array([rng.choice(np.nonzero(m)[0]) if m.any() else 0 for m in legal]))
        if t % 6 == 5:
            got = env.refill_census()
            assert set(got) == {"count", "solvable_fraction", "hazard"}
            count, _ = CR.oracle_census(env.dev.state()["board"])
            assert got["count"].tolist() == count.tolist()
            assert np.array_equal(got["solvable_fraction"], count / CR.NUM_HANDS)
            assert np.array_equal(got["hazard"], K.refill_hazard(torch.from_numpy(count)).numpy())
    env.close()

    one = BlockBlastEnv(seed=5, device="cpu")
    one.reset()
    for t in range(12):
        one.step(one.sample_valid_action())
    got = one.refill_census()
    count, _ = CR.oracle_census(one._dev.state()["board"])
    assert got == {"count": int(count[0]), "solvable_fraction": int(count[0]) / CR.NUM_HANDS,
                   "hazard": float(K.refill_hazard(torch.from_numpy(count))[0])}
    one.close()
