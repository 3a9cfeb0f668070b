#!/usr/bin/env python3
"""Time the per-action values and the dealt next-hand values with the shape terms against the kernels they extend.

The protocol of tools/bench_eval_terms.py: mid-game positions (seeds 7 + i after 40 steps of random legal play),
depth 3, one process, device events, the variants interleaved round by round so that clock and thermal drift meets
them alike.  The yardsticks are the existing kernels in the same process.  Per batch size

  plan values    bb_plan_values_pos under the default weights (the yardstick), against bb_plan_values_ext_pos with
                 per-position rows whose four shape weights are 0 (ext_zero), with perimeter, room3 and room5 set
                 (ext_prr) and with all four set (ext_all); all four outputs written
  refill values  bb_refill_values_pos (the yardstick) against bb_refill_values_ext_pos under the same three rows, 16
                 deals per board (value alone, as the two-hand agent asks)

Prints one JSON line: per variant the median, minimum and maximum in milliseconds over the rounds and the ratio of
each ext median to its yardstick's; writes it to --output too.

    python tools/bench_values_ext.py --rounds 15 --output profiles/values_ext/bench_run1.json
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def mid_game(n, steps, seed0, dev):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(n, [seed0 + i for i in range(n)], device=dev)
    env.reset()
    mb = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    a0 = torch.zeros(n, dtype=torch.int32, device=dev)
    env.obs(mask_bits=mb)
    env.random_actions(mb, a0, step=0)
    env.rollout(steps, a0, torch.zeros((steps, n), device=dev), torch.zeros((steps, n), dtype=torch.uint8, device=dev))
    env.sync()
    st = env.state()
    env.close()
    return (torch.from_numpy(st["board"].view(np.int64).copy()).to(dev),
            torch.from_numpy(st["hand"].view(np.int32).copy()).to(dev), torch.from_numpy(st["combo"].copy()).to(dev))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def interleaved(variants, warmup, rounds, yardstick):
    ms = {k: [] for k in variants}
    for rnd in range(warmup + rounds):
        for k, fn in variants.items():
            t = timed(fn)
            if rnd >= warmup:
                ms[k].append(t)
    res = {k: summary(v) for k, v in ms.items()}
    for k in variants:
        if k != yardstick:
            res[k][f"ratio_to_{yardstick}"] = res[k]["median_ms"] / res[yardstick]["median_ms"]
    return res


def main():
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K
    from runtime import lib as L

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--deals", type=int, default=16)
    ap.add_argument("--output", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    prr = {**DEFAULT_WEIGHTS, "perimeter": -3, "room3": 4, "room5": 2}
    sets = {"ext_zero": dict(DEFAULT_WEIGHTS), "ext_prr": prr, "ext_all": {**prr, "fits": 25}}
    rec = {"record": "bench_values_ext", "depth": 3, "deals": args.deals, "build_id": L.build_id(),
           "device": torch.cuda.get_device_name(0), "plan_values": {}, "refill_values": {}}
    for n in args.sizes:
        board, hand, combo = mid_game(n, 40, 7, dev)
        pv = K.plan_value_outputs(n, dev)
        variants = {"plan_values": lambda: K.plan_values(board, hand, DEFAULT_WEIGHTS, 3, combo=combo, out=pv)}
        rv = K.refill_value_outputs(n, args.deals, dev)
        refills = {"refill_values": lambda: K.refill_values(board, DEFAULT_WEIGHTS, args.deals, 1, combo=combo, depth=3,
                                                            out=rv)}
        for name, w in sets.items():
            rows = K.eval_rows(w, n=n, device=dev)
            variants[name] = (lambda r: lambda: K.plan_values_ext(board, hand, r, 3, combo=combo, out=pv))(rows)
            refills[name] = (lambda r: lambda: K.refill_values_ext(board, r, args.deals, 1, combo=combo, depth=3,
                                                                   out=rv))(rows)
        res = interleaved(variants, args.warmup, args.rounds, "plan_values")
        res["leaves_total"] = int(pv["leaves"].sum())
        rec["plan_values"][str(n)] = res
        res = interleaved(refills, args.warmup, args.rounds, "refill_values")
        res["pairs"] = n * args.deals
        rec["refill_values"][f"{n}x{args.deals}"] = res
    line = json.dumps(rec)
    print(line)
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
