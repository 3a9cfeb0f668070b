#!/usr/bin/env python3
"""Diagnostics (not product): per-launch time of the refill census (census_kernel in csrc/bb_census.hip,
bb_refill_census_pos, count only) against what the library could do without it, on the same build.

Reported per board set (one JSON line; --out FILE also writes it):
  new      bb_refill_census_pos, count only, one launch
  chain    bb_safe_mask_pos mode 0 on the 9,139 x n replicated (board, hand) pairs, then the weighted count in torch
           (a hand counts with its multiplicity 6 / 3 / 1 where any first move is safe); the replicas are built
           outside the timed region
  equal    both give the same counts, checked before anything is timed
  bar_met  the slowest repeat of `new` is below the fastest repeat of `chain`
  chain_over_new   ratio of the medians
The sets: mid-game boards (seeds 7 + i after 40 bb_rollout steps, as tools/bench_plan.py takes them) at three sizes,
boards of tests/_safe_positions.crowded's kind, and empty boards.  --tuner adds the wall time of a 2-generation
tuner run with and without the census (fitness "survival" against "score").
Timing as tools/bench_plan.py: device events around back-to-back launches, warm-up first, `reps` repeats
interleaved between the candidates in one process; median, minimum and maximum.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_plan import played, timed  # noqa: E402
from runtime import kernels as K  # noqa: E402

MULTISETS = np.array(list(itertools.combinations_with_replacement(range(37), 3)), np.int64)
HAND_WORDS = (MULTISETS[:, 0] | MULTISETS[:, 1] << 6 | MULTISETS[:, 2] << 12).astype(np.int32)
MULTIPLICITY = np.array([{3: 6, 2: 3, 1: 1}[len(set(m))] for m in MULTISETS.tolist()], np.int64)


def crowded_boards(n, seed=2024, fills=(0.35, 0.5, 0.6, 0.7, 0.8, 0.9)):
    """tests/_safe_positions.crowded's boards: random fill 0.35 .. 0.9, no full line."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, np.uint64)
    for i in range(n):
        g = rng.random((8, 8)) < fills[i % 6]
        for r in range(8):
            if g[r].all():
                g[r, rng.integers(8)] = False
        for c in range(8):
            if g[:, c].all():
                g[rng.integers(8), c] = False
        out[i] = sum(1 << (r * 8 + c) for r in range(8) for c in range(8) if g[r, c])
        rng.integers(0, 37, 3)  # the hand crowded() draws here: the same boards as the tests'
    return out


def measure(board, inner_new, inner_chain, reps, warmup):
    """One board set: the repeats of the two candidates interleaved, each with its own launches per repeat."""
    n, dev = board.numel(), board.device
    m = len(MULTISETS)
    rep_board = board.repeat_interleave(m)
    rep_hand = torch.from_numpy(HAND_WORDS).to(dev).repeat(n)
    mult = torch.from_numpy(MULTIPLICITY).to(dev)
    words = torch.zeros((n * m, 3), dtype=torch.int64, device=dev)
    new = {"count": torch.zeros(n, dtype=torch.int32, device=dev)}
    chained = torch.zeros(n, dtype=torch.int64, device=dev)

    def chain():
        K.safe_mask(rep_board, rep_hand, K.SAFE_WORDS, out=words)
        chained.copy_(((words != 0).any(dim=1).view(n, m) * mult).sum(dim=1))

    def new_many():
        for _ in range(inner_new):
            K.refill_census(board, out=new)

    def chain_many():
        for _ in range(inner_chain):
            chain()

    chain()
    K.refill_census(board, out=new)
    if not torch.equal(new["count"].long(), chained):
        sys.exit(f"bench_refill_census: the counts differ on {n} boards")
    r = timed({"new": new_many, "chain": chain_many}, 1, reps, warmup)
    for k, inner in (("new", inner_new), ("chain", inner_chain)):
        r[k] = {key: round(v / inner, 5) for key, v in r[k].items()}
    frac = new["count"].double() / K.NUM_HANDS
    return {"boards": n, "equal": True, "mean_solvable_fraction": round(float(frac.mean()), 4),
            "min_solvable_fraction": round(float(frac.min()), 4), **r,
            "bar_met": r["new"]["max_ms"] < r["chain"]["min_ms"],
            "chain_over_new": round(r["chain"]["median_ms"] / r["new"]["median_ms"], 1)}


def tuner_walls():
    from evaluation.tune import tune

    out = {}
    for fitness in ("score", "survival", "score", "survival"):  # the first pair warms both paths up
        t0 = time.perf_counter()
        tune(generations=2, fitness=fitness)
        torch.cuda.synchronize()
        out[fitness] = round(time.perf_counter() - t0, 3)
    return {"census_false_s": out["score"], "census_true_s": out["survival"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, nargs="*", default=[64, 512, 4096])
    ap.add_argument("--crowded", type=int, default=512)
    ap.add_argument("--empty", type=int, default=512)
    ap.add_argument("--play", type=int, default=40, help="rollout steps played before the boards are taken")
    ap.add_argument("--inner", type=int, default=10, help="launches of the census per repeat")
    ap.add_argument("--inner-chain", type=int, default=1, help="runs of the chain per repeat")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tuner", action="store_true", help="also time a 2-generation tuner run with and without the census")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_refill_census: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    out = {"played_steps": args.play, "inner": args.inner, "inner_chain": args.inner_chain, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "build_id": K.L.build_id()}
    sets = []
    for count in args.mid:
        env = played(count, args.play, dev)
        sets.append((f"mid_{count}", torch.from_numpy(env.state()["board"].view(np.int64).copy()).to(dev)))
        env.close()
    if args.crowded:
        sets.append((f"crowded_{args.crowded}",
                     torch.from_numpy(crowded_boards(args.crowded).view(np.int64).copy()).to(dev)))
    if args.empty:
        sets.append((f"empty_{args.empty}", torch.zeros(args.empty, dtype=torch.int64, device=dev)))
    for key, board in sets:
        out[key] = measure(board, args.inner, args.inner_chain, args.reps, args.warmup)
        print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    if args.tuner:
        out["tuner_2_generations"] = tuner_walls()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
