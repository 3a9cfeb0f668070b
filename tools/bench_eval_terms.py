#!/usr/bin/env python3
"""Time the search with the shape terms against the per-position search it extends.

Mid-game positions (random legal play from seeded games), depth 3, one process, the variants interleaved round by
round so that clock and thermal drift meets them alike.  Per batch size the launches timed with device events are

  each      bb_plan_actions_each_pos under the default weights (the yardstick)
  ext_zero  bb_plan_actions_ext_pos, the four shape weights 0
  ext_prr   ... perimeter, room3 and room5 set
  ext_all   ... all four set

and bb_board_terms_pos on 65,536 boards.  Prints one JSON line: per variant the median, minimum and maximum in
milliseconds over the rounds, and the ratio of each ext median to the yardstick's; writes it to --output too.

    python tools/bench_eval_terms.py --rounds 15 --output profiles/eval_terms/bench_run1.json
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


def main():
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K
    from runtime import lib as L

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--output", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    prr = {**DEFAULT_WEIGHTS, "perimeter": -3, "room3": 4, "room5": 2}
    sets = {"ext_zero": dict(DEFAULT_WEIGHTS), "ext_prr": prr, "ext_all": {**prr, "fits": 25}}
    rec = {"record": "bench_eval_terms", "depth": 3, "build_id": L.build_id(), "device": torch.cuda.get_device_name(0),
           "sizes": {}}
    for n in args.sizes:
        board, hand, combo = mid_game(n, 40, 7, dev)
        out = {"action": torch.empty(n, dtype=torch.int32, device=dev),
               "leaves": torch.empty(n, dtype=torch.int32, device=dev)}
        each_rows = K.weight_rows(DEFAULT_WEIGHTS, n=n, device=dev)
        variants = {"each": lambda: K.plan_actions_each(board, hand, each_rows, 3, combo=combo, want_value=False, **out)}
        for name, w in sets.items():
            rows = K.eval_rows(w, n=n, device=dev)
            variants[name] = (lambda r: lambda: K.plan_actions_ext(board, hand, r, 3, combo=combo, want_value=False,
                                                                   **out))(rows)
        ms = {k: [] for k in variants}
        for rnd in range(args.warmup + args.rounds):
            for k, fn in variants.items():
                t = timed(fn)
                if rnd >= args.warmup:
                    ms[k].append(t)
        res = {k: summary(v) for k, v in ms.items()}
        for k in sets:
            res[k]["ratio_to_each"] = res[k]["median_ms"] / res["each"]["median_ms"]
        res["leaves_total"] = int(out["leaves"].sum())
        rec["sizes"][str(n)] = res
    boards = torch.from_numpy(np.random.default_rng(3).integers(0, 2 ** 63, 65536, dtype=np.int64)).to(dev)
    terms = torch.empty((65536, 4), dtype=torch.int32, device=dev)
    ms = [timed(lambda: K.board_terms(boards, out=terms)) for _ in range(args.warmup + args.rounds)][args.warmup:]
    rec["board_terms_65536"] = summary(ms)
    line = json.dumps(rec)
    print(line)
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
