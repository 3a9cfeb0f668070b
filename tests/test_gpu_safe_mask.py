"""The hand-safe mask call on the MI355X (safe_mask_kernel in csrc/bb_lookahead.hip: bb_safe_mask / bb_safe_mask_pos).

* A graph capture of this file's first bb_safe_mask launch (this test comes first), replayed on changed columns.
* Against the references of tests/_safe_positions.py (which call neither entry point): the 92-position set at
  n = 1, 5 and 67, stateless and handle form, both modes; the crowded set.
* Against the host backend and against HIP bb_plan_values' safe words at the 1,031 mid-game positions of
  tests/test_gpu_plan.py; on three fresh boards.
* Above the grid cap: 4 * 32,768 + 3 positions, so the first three waves of workgroup 0 take a second position; one
  of each such pair is crafted to take the fallback of mode 1 and the other is a played position.
* The handle form leaves every state column and the RNG unchanged.
"""
import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _safe_positions as S
from test_gpu_plan import N_MID, _rolled, _subset

pytestmark = pytest.mark.gpu

SAFE_WAVES, SAFE_MAX_GRID = 4, 1 << 15  # kSafeWaves, kSafeMaxGrid of csrc/bb_lookahead.hip
FILL = -7


def _host_mask(board, hand, mode):
    from runtime import kernels as K
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    b, h = S.tensors(board, hand, torch.device("cpu"))
    return S.as_u64(K.safe_mask(b, h, mode))


def test_graph_capture_of_the_first_call_and_replays(cuda):
    """No eager bb_safe_mask launch precedes the capture in this file.  Both modes are captured in one graph, which
    is replayed three times, the position columns rewritten in place before the second and third."""
    from runtime import kernels as K

    a = S.reference_a()
    n = 23
    sets = [np.arange(k, k + n) for k in (0, 30, 69)]
    board, hand = S.tensors(a["board"][sets[0]], a["hand"][sets[0]], cuda)
    o0 = torch.full((n, 3), FILL, dtype=torch.int64, device=cuda)
    o1 = torch.full((n, 3), FILL, dtype=torch.int64, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.safe_mask(board, hand, 0, out=o0)
        K.safe_mask(board, hand, 1, out=o1)
    for idx in sets:
        b, h = S.tensors(a["board"][idx], a["hand"][idx], cuda)
        board.copy_(b), hand.copy_(h)
        o0.fill_(FILL), o1.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        S.assert_words(o0, a["safe"][idx], f"graph replay mode 0 on positions {idx[0]}..")
        S.assert_words(o1, a["mode1"][idx], f"graph replay mode 1 on positions {idx[0]}..")
    assert (a["mode1"][sets[2]] != a["safe"][sets[2]]).any()  # the last window holds the crafted fallback position


@pytest.mark.parametrize("n", [1, 5, 67])
def test_reference_a_both_forms_both_modes(cuda, n):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    ref, a = R.reference(), S.reference_a()
    idx = _subset(ref, n)
    board, hand = S.tensors(a["board"][idx], a["hand"][idx], cuda)
    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device=cuda)
    env.reset()
    R.set_positions(env, [ref["envs"][i] for i in idx])
    for mode, key in ((0, "safe"), (1, "mode1")):
        S.assert_words(K.safe_mask(board, hand, mode), a[key][idx], f"_pos n={n} mode={mode}")
        out = torch.full((n, 3), FILL, dtype=torch.int64, device=cuda)
        env._safe_mask(mode, out)
        S.assert_words(out, a[key][idx], f"handle n={n} mode={mode}")
    env.close()


def test_crowded_set(cuda):
    from runtime import kernels as K

    b = S.reference_b()
    board, hand = S.tensors(b["board"], b["hand"], cuda)
    S.assert_words(K.safe_mask(board, hand, 0), b["safe"], "crowded mode 0")
    S.assert_words(K.safe_mask(board, hand, 1), b["mode1"], "crowded mode 1")
    S.assert_words(K.safe_mask(board, hand, 0), _host_mask(b["board"], b["hand"], 0), "crowded mode 0 against the host")
    S.assert_words(K.safe_mask(board, hand, 1), _host_mask(b["board"], b["hand"], 1), "crowded mode 1 against the host")


def test_mid_game_equals_host_and_plan_values(cuda):
    env = _rolled(N_MID, 40, 7, cuda)
    st = env.state()
    safe_pv = env.plan_values({}, 2, out={"safe": torch.full((N_MID, 3), FILL, dtype=torch.int64, device=cuda)})["safe"]
    host_safe, host_legal = S.host_safe_legal(st["board"], st["hand"])  # the host's bb_plan_values
    S.assert_words(safe_pv, host_safe, "HIP bb_plan_values safe against the host's")
    out = torch.full((N_MID, 3), FILL, dtype=torch.int64, device=cuda)
    S.assert_words(env.safe_mask(out, depth=3), host_safe, "mode 0 against bb_plan_values (host)")
    assert torch.equal(out, safe_pv)
    S.assert_words(out, _host_mask(st["board"], st["hand"], 0), "mode 0 against the host's bb_safe_mask")
    env.sampling_mask(out)
    S.assert_words(out, S.sampling(host_safe, host_legal), "mode 1 against bb_plan_values (host)")
    S.assert_words(out, _host_mask(st["board"], st["hand"], 1), "mode 1 against the host's bb_safe_mask")
    legal_col = torch.zeros_like(out)
    env.obs(mask_bits=legal_col)
    S.assert_words(legal_col, host_legal, "the env's mask column against the legal words")
    unsafe = int(S.V.safe_bool(host_legal & ~host_safe).sum())
    assert unsafe > 0
    print(f"mid-game: {int(S.V.safe_bool(host_legal).sum())} legal actions, {unsafe} unsafe")
    env.close()


def test_fresh_boards(cuda):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(3, [7, 8, 9], autoreset=False, device=cuda)
    env.reset()
    st = env.state()
    assert (st["board"] == 0).all()
    _, legal = S.host_safe_legal(st["board"], st["hand"])
    for mode in (0, 1):
        out = torch.full((3, 3), FILL, dtype=torch.int64, device=cuda)
        env._safe_mask(mode, out)
        S.assert_words(out, legal, f"fresh boards: every legal move is safe (mode {mode})")
    env.close()


def test_more_positions_than_waves(cuda):
    """n = 4 * the grid cap + 3 = 131,075, every game from its own seed: waves 0..2 of workgroup 0 take a second
    position.  Positions 0..2 are overwritten with crafted positions that have legal moves and none safe (the
    fallback of mode 1), so the two positions of such a wave differ in their safe words and in the branch they
    take; a wave that kept anything of its first position would show in the second."""
    from runtime import kernels as K

    stride = SAFE_WAVES * SAFE_MAX_GRID
    n = stride + 3
    assert n == 131075
    env = _rolled(n, 25, 1000, cuda)
    st = env.state()
    env.close()
    board, hand = st["board"].copy(), st["hand"].copy()
    a = S.reference_a()
    fb = np.nonzero((a["safe"] == 0).all(axis=1) & (a["legal"] != 0).any(axis=1))[0]
    crafted = np.resize(fb, 3)
    board[:3], hand[:3] = a["board"][crafted], a["hand"][crafted]
    want0, want1 = _host_mask(board, hand, 0), _host_mask(board, hand, 1)
    for i in range(3):
        assert (want0[i] == 0).all() and (want1[i] != 0).any()                       # the fallback
        assert (want0[i + stride] != 0).any() and (want0[i + stride] != want0[i]).any()  # the wave's second position
    assert ((want0[1:] != want0[:-1]).any(axis=1)).mean() > 0.9  # neighbours differ too
    b, h = S.tensors(board, hand, cuda)
    S.assert_words(K.safe_mask(b, h, 0), want0, "above the grid cap, mode 0")
    S.assert_words(K.safe_mask(b, h, 1), want1, "above the grid cap, mode 1")


def test_handle_leaves_the_state_and_rng_unchanged(cuda):
    env = _rolled(257, 30, 500, cuda)
    before = env.state()
    out = torch.zeros((257, 3), dtype=torch.int64, device=cuda)
    for mode in (0, 1, 1, 0):
        env._safe_mask(mode, out)
    torch.cuda.synchronize()
    after = env.state()
    assert "rng" in before
    for k in before:
        assert np.array_equal(before[k], after[k]), f"state {k} changed"
    # and the games go on as if it had not been called: the same next step as an untouched twin
    twin = _rolled(257, 30, 500, cuda)
    act = torch.zeros(257, dtype=torch.int32, device=cuda)
    env.random_actions(out, act, step=99)
    for e in (env, twin):
        e.step(act)
    a, b = env.state(), twin.state()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"state {k} differs from the twin's after a step"
    env.close()
    twin.close()
