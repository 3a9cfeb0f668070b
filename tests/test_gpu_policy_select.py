"""The policy's bit select on the GPU (csrc/bb_device.h select_bit through random_policy) against the host
backend, whose plain-loop select shares nothing with that header: ``DeviceEnvBatch.random_actions`` on 4,096
hand-made mask rows, equal bit for bit at two policy steps.

The rows: the 192 single-bit masks, all ones, each word alone, high halves only, low halves only, alternating
bits both ways, the empty mask (action 0), and random rows of densities 1/64 .. 63/64.  From the expected
(host) output the test also shows that the rows exercise the search: every action occurs, and in either 32-bit
half every one of the five levels goes both ways (bit b of the position inside the half is the outcome of
``k >= count`` at level 1 << b)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096
SEED = 0xB10C
STEPS = (0, 7)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _rows():
    m = np.zeros((N, 3), dtype=np.uint64)
    r = 0
    for a in range(192):  # the single-bit masks: the only legal action is a
        m[r, a // 64] = np.uint64(1) << np.uint64(a % 64)
        r += 1
    m[r] = ONES
    r += 1
    for w in range(3):  # one word only
        m[r, w] = ONES
        r += 1
    m[r] = np.uint64(0xFFFFFFFF00000000)
    m[r + 1] = np.uint64(0x00000000FFFFFFFF)
    m[r + 2] = np.uint64(0xAAAAAAAAAAAAAAAA)
    m[r + 3] = np.uint64(0x5555555555555555)
    r += 4
    empty = r  # stays zero
    r += 1
    rng = np.random.default_rng(14)
    dens = (np.arange(N - r) % 63 + 1) / 64.0
    bits = rng.random((N - r, 192)) < dens[:, None]
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    m[r:] = (bits.reshape(N - r, 3, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)
    return m, empty


def _actions(device, masks, step):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(N, seeds=list(range(N)), device=device)
    mb = torch.from_numpy(masks.view(np.int64)).to(env.device)
    out = torch.full((N,), -1, dtype=torch.int32, device=env.device)
    env.random_actions(mb, out, seed=SEED, step=step)
    if env.device.type == "cuda":
        torch.cuda.synchronize()
    res = out.cpu().numpy().copy()
    env.close()
    return res


@pytest.fixture(scope="module")
def rows():
    return _rows()


@pytest.fixture(scope="module")
def expected(rows):
    return {step: _actions("cpu", rows[0], step) for step in STEPS}


@pytest.mark.parametrize("step", STEPS)
def test_gpu_select_equals_host_select(cuda, rows, expected, step):
    got = _actions(cuda, rows[0], step)
    want = expected[step]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), [hex(int(w)) for w in rows[0][i]], int(got[i]), int(want[i])) for i in bad[:8]]


def test_rows_exercise_every_level(rows, expected):
    masks, empty = rows
    for step in STEPS:
        act = expected[step].astype(np.int64)
        assert np.array_equal(act[:192], np.arange(192))  # the single-bit rows: every action occurs
        assert act[empty] == 0 and not masks[empty].any()
        full = np.flatnonzero(masks.any(axis=1))
        a = act[full]
        assert ((masks[full, a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).all()  # a legal action each
        half, pos = (a % 64) // 32, a % 32
        for h in (0, 1):
            for b in range(5):
                seen = set(((pos[half == h] >> b) & 1).tolist())
                assert seen == {0, 1}, (step, h, b, seen)
