#!/usr/bin/env python3
"""Diagnostics (not product): per-launch time of the sampling mask (safe_mask_kernel in csrc/bb_lookahead.hip,
bb_safe_mask mode 1) against the chain it replaces on the same build, on the positions of tools/bench_plan.py: N
mid-game positions from a played-in rollout, a bigger such set, and fresh boards.

Reported per position set (one JSON line; --out FILE also writes it):
  new      bb_safe_mask, mode BB_SAFE_OR_LEGAL, one launch
  words    bb_safe_mask, mode BB_SAFE_WORDS (what DeviceEnvBatch.safe_mask now launches)
  chain    bb_plan_values with the safe words alone at depth 2, then the three torch ops of
           agents.greedy.apply_safe_mask on a copy of the env's legal words (the copy is part of neither)
  equal    the new call's words equal the chain's (and mode 0 the safe words of bb_plan_values), checked before
           anything is timed
  bar_met  the slowest repeat of `new` is below the fastest repeat of `chain`
  chain_over_new   ratio of the medians
  regs     VGPRs / SGPRs / LDS / scratch of the kernels from the code object's metadata
Timing as tools/bench_plan.py: device events around back-to-back launches, warm-up first, `reps` repeats
interleaved between the candidates in one process; median, minimum and maximum.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lookahead import code_object_metadata  # noqa: E402
from bench_plan import played, timed  # noqa: E402
from runtime import kernels as K  # noqa: E402


def measure(env, inner, reps, warmup):
    n, dev = env.num_envs, env.device
    legal = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    env.obs(mask_bits=legal)
    safe = {"safe": torch.zeros((n, 3), dtype=torch.int64, device=dev)}
    chained = torch.zeros_like(legal)
    new = torch.zeros_like(legal)
    words = torch.zeros_like(legal)

    def chain():  # agents.greedy.apply_safe_mask with bb_plan_values behind it, written out
        env.plan_values({}, 2, out=safe)
        has_safe = (safe["safe"] != 0).any(dim=1, keepdim=True)
        chained.copy_(torch.where(has_safe, legal & safe["safe"], legal))

    chain()
    env.sampling_mask(new)
    env._safe_mask(0, words)
    equal = {"mode1": bool(torch.equal(new, chained)), "mode0": bool(torch.equal(words, safe["safe"]))}
    if not all(equal.values()):
        sys.exit(f"bench_safe_mask: results differ on {n} positions: {equal}")
    r = timed({"new": lambda: env.sampling_mask(new), "chain": chain, "words": lambda: env._safe_mask(0, words)},
              inner, reps, warmup)
    fallback = int(((safe["safe"] == 0).all(dim=1) & (legal != 0).any(dim=1)).sum())
    return {"positions": n, "equal": equal, "fallback_positions": fallback, **r,
            "bar_met": r["new"]["max_ms"] < r["chain"]["min_ms"],
            "chain_over_new": round(r["chain"]["median_ms"] / r["new"]["median_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--fresh", type=int, default=4096)
    ap.add_argument("--play", type=int, default=40, help="rollout steps played before the positions are taken")
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-regs", action="store_true", help="skip the compile that reads the code object's metadata")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_safe_mask: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    out = {"played_steps": args.play, "inner": args.inner, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "build_id": K.L.build_id()}
    for key, count, steps in (("mid", args.positions, args.play), ("mid_big", args.big, args.play),
                              ("fresh", args.fresh, 0)):
        if count:
            env = played(count, steps, dev)
            out[key] = measure(env, args.inner, args.reps, args.warmup)
            env.close()
    if not args.no_regs:
        out["regs"] = code_object_metadata()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
