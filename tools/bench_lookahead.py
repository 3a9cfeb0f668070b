#!/usr/bin/env python3
"""Diagnostics (not product): per-launch time of the one-ply lookahead kernels (csrc/bb_lookahead.hip) at N
positions taken from a played-in rollout.

Reported (one JSON line; --out FILE also writes it):
  afterstates_ms      bb_afterstates with all four outputs
  afterstates_hbm     its share of HBM bandwidth by its own byte contract: 24 B x 192 written per position, over
                      the measured time, against 8.0 TB/s (spec) and 6.3 TB/s (the achievable copy rate)
  greedy_ms           bb_greedy_actions (action + value)
  dense_argmax_ms     what the fused kernel replaces: bb_afterstates (board + score + aux; the value needs no
                      reward) followed by a torch arg-max over the value built from those outputs
  greedy_regs         VGPRs / SGPRs / LDS / occupancy of the two kernels, read from the code object's metadata
                      (the assembly hipcc makes from the sources with the build's flags; needs no GPU)
Timing: device events around `inner` back-to-back launches, warm-up first, `reps` repeats interleaved between the
candidates in one process; the median and the minimum of the repeats are reported.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"))
from runtime import build as B  # noqa: E402
from runtime import kernels as K  # noqa: E402
from runtime.device_env import DeviceEnvBatch  # noqa: E402

WEIGHTS = {"lines": 100, "score": 0, "holes": -30, "filled": -2, "centre": 0, "mobility": 1, "dead": -100000,
           "refill": 0}
FIELDS = ("lines", "score", "holes", "filled", "centre", "mobility", "dead", "refill")


def code_object_metadata():
    """Registers, LDS and waves per SIMD of the lookahead kernels from the metadata of the gfx950 assembly."""
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    out = os.path.join(tempfile.mkdtemp(), "look.s")
    subprocess.run([B._hipcc(), *flags, f"-I{os.path.join(REPO, 'include')}", "--cuda-device-only", "-S", "-o", out,
                    os.path.join(B.CSRC, "bb_lookahead.hip")], check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    res = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = next(k for k in ("greedy_kernel", "greedy_each_kernel", "afterstates_kernel", "plan_kernel",
                                "plan_each_kernel", "plan_values_kernel", "safe_mask_kernel")
                     if k in name)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        res[short] = {
            "vgpr": vgpr, "sgpr": int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1)),
            "lds_bytes": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)),
            "scratch_bytes": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
            # gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves per SIMD
            "waves_per_simd": min(8, 512 // (-(-vgpr // 8) * 8)),
        }
    return res


def timed(fns, inner, reps, warmup):
    """ms per launch of each fn: events around `inner` launches, the candidates interleaved over `reps` rounds."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=65536)
    ap.add_argument("--play", type=int, default=40, help="rollout steps played before the positions are taken")
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lookahead: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    n = args.positions
    env = DeviceEnvBatch(n, [7 + i for i in range(n)], device=dev)
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    a0 = torch.zeros(n, dtype=torch.int32, device=dev)
    env.obs(mask_bits=mb)
    env.random_actions(mb, a0, step=0)
    env.rollout(args.play, a0, torch.zeros((args.play, n), device=dev),
                torch.zeros((args.play, n), dtype=torch.uint8, device=dev))
    env.sync()

    full = K.afterstate_outputs(n, dev)
    part = K.afterstate_outputs(n, dev, want=("board", "score_gained", "aux"))
    act = torch.zeros(n, dtype=torch.int32, device=dev)
    val = torch.zeros(n, dtype=torch.int64, device=dev)
    w = K.L.greedy_weights(WEIGHTS)

    def dense_argmax():
        env.afterstates(out=part)
        f = K.unpack_aux(part["aux"])
        f["score"] = part["score_gained"].long()
        b = part["board"]
        b = b - ((b >> 1) & 0x5555555555555555)  # popcount of the board bits
        b = (b & 0x3333333333333333) + ((b >> 2) & 0x3333333333333333)
        b = (b + (b >> 4)) & 0x0F0F0F0F0F0F0F0F
        f["filled"] = ((b * 0x0101010101010101) >> 56) & 0xFF
        v = sum(WEIGHTS[k] * f[k].long() for k in FIELDS if WEIGHTS[k])
        v = torch.where(f["legal"], v, torch.full_like(v, -(2 ** 63)))
        return v.argmax(dim=1)

    # the two ways to the greedy action agree wherever the maximum is unique (torch's argmax does not promise
    # the lowest index on ties), before anything is timed
    env.greedy_actions(act, w, value=val)
    ref = dense_argmax()
    legal_any = K.unpack_aux(part["aux"])["legal"].any(dim=1)
    agree = float(((act.long() == ref) | ~legal_any).float().mean())

    res = timed({"afterstates": lambda: env.afterstates(out=full),
                 "greedy": lambda: env.greedy_actions(act, w, value=val),
                 "dense_argmax": dense_argmax}, args.inner, args.reps, args.warmup)
    bytes_per_launch = n * 192 * 24
    t = res["afterstates"]["median_ms"] * 1e-3
    out = {
        "positions": n, "played_steps": args.play, "inner": args.inner, "reps": args.reps,
        "device": torch.cuda.get_device_name(0), "build_id": K.L.build_id(),
        "afterstates_ms": res["afterstates"], "greedy_ms": res["greedy"], "dense_argmax_ms": res["dense_argmax"],
        "afterstates_bytes": bytes_per_launch,
        "afterstates_hbm": {"TB_per_s": round(bytes_per_launch / t / 1e12, 3),
                            "of_8.0_spec": round(bytes_per_launch / t / 8.0e12, 3),
                            "of_6.3_achievable": round(bytes_per_launch / t / 6.3e12, 3)},
        "fused_speedup_over_dense_argmax": round(res["dense_argmax"]["median_ms"] / res["greedy"]["median_ms"], 2),
        "greedy_agrees_with_dense_argmax": agree,
        "greedy_regs": code_object_metadata(),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
