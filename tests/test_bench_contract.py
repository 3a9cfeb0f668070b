"""bench.py's launch contract on the host (no GPU): `--gpus N` must run N ranks.

A rank whose WORLD_SIZE disagrees with --gpus exits non-zero before touching
the GPU; a plain `--gpus N` (no WORLD_SIZE) hands over to torch.distributed.run
with N ranks of the same command line (tests/test_gpu_full_size.py runs it for
real on the GPU box).
"""
import importlib.util
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mismatched_world_size_fails():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr[-2000:]
    assert "WORLD_SIZE=3" in r.stderr


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_formats_and_sample(tmp_path, monkeypatch):
    """--dump-outputs' writer on the host backend: float32 / float64 arrays of the last launch's outputs, every
    env when they fit the byte budget, else a fixed sample of envs (the same on every call) named in env_index;
    the 64-bit mask words survive as exact 32-bit halves."""
    import numpy as np
    import torch

    bench = _bench_module()
    from runtime.device_env import DeviceEnvBatch

    n, T, S = 96, 8, 2
    ns = n // S
    shards = []
    for k in range(S):
        e = DeviceEnvBatch(ns, seeds=[42 + k * ns + i for i in range(ns)], device="cpu", env_offset=k * ns)
        e.reset()
        mb = torch.zeros((ns, 3), dtype=torch.int64)
        e.obs(mask_bits=mb)
        a = [torch.zeros(ns, dtype=torch.int32), torch.zeros(ns, dtype=torch.int32)]
        e.random_actions(mb, a[0], seed=bench.POLICY_SEED, step=0)
        outs = (torch.zeros((T, ns)), torch.zeros((T, ns), dtype=torch.uint8), torch.zeros((T, ns), dtype=torch.uint8),
                torch.zeros((T, ns), dtype=torch.int32), torch.zeros((T, ns, 3), dtype=torch.int64))
        e.rollout(T, a[0], outs[0], outs[1], lines=outs[2], actions_out=outs[3], mask_out=outs[4], next_action=a[1],
                  policy_seed=bench.POLICY_SEED, policy_step0=0)
        a.reverse()
        shards.append((e, None, a, outs))
    whole = [torch.cat([sh[3][j] for sh in shards], dim=1).numpy() for j in range(5)]
    nxt = torch.cat([sh[2][0] for sh in shards]).numpy()

    def check(path, idx):
        got = {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}
        assert sorted(got) == ["actions", "env_index", "lines", "mask_words", "next_action", "reward", "terminated"]
        assert all(v.dtype in (np.float32, np.float64) for v in got.values())
        assert np.array_equal(got["env_index"], idx)
        for j, name in enumerate(("reward", "terminated", "lines", "actions")):
            assert np.array_equal(got[name], whole[j][:, idx].astype(np.float32)), name
        assert np.array_equal(got["next_action"], nxt[idx].astype(np.float32))
        w = got["mask_words"].astype(np.uint64)
        assert np.array_equal((w[..., 0::2] | (w[..., 1::2] << np.uint64(32))).view(np.int64), whole[4][:, idx])
        return got

    bench.dump_outputs(str(tmp_path / "all"), shards, "rollout", T, 0, False)
    check(str(tmp_path / "all"), np.arange(n))
    per_env = T * (4 * 4 + 6 * 8) + 4 + 8
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40 * per_env)  # room for 40 of the 96 envs
    bench.dump_outputs(str(tmp_path / "s1"), shards, "rollout", T, 0, False)
    bench.dump_outputs(str(tmp_path / "s2"), shards, "rollout", T, 0, False)
    idx = np.load(str(tmp_path / "s1" / "env_index.npy")).astype(np.int64)
    assert len(idx) == 40 and len(set(idx)) == 40 and (np.diff(idx) > 0).all() and idx.max() < n
    assert np.array_equal(idx, np.load(str(tmp_path / "s2" / "env_index.npy")))  # the same sample every time
    check(str(tmp_path / "s1"), idx)
    bench.dump_outputs(str(tmp_path / "step"), shards, "step", T, 1, False)  # step mode, rank 1's file names
    assert sorted(os.listdir(tmp_path / "step")) == ["env_index_rank1.npy", "next_action_rank1.npy",
                                                     "reward_rank1.npy", "terminated_rank1.npy"]
    for sh in shards:
        sh[0].close()


def test_gpus_flag_relaunches(monkeypatch):
    bench = _bench_module()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    import subprocess as sp

    monkeypatch.setattr(sp, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 7  # the child's exit code
    else:
        raise AssertionError("bench.main() did not exit with the launcher's code")
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert "--master-addr=127.0.0.1" in cmd and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
