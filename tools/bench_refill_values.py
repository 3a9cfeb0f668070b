#!/usr/bin/env python3
"""Diagnostics (not product): per-launch time of the dealt next-hand values (refill_values_kernel in
csrc/bb_lookahead.hip, bb_refill_values_pos, value only) against the search alone on the same build.

Reported per board set (one JSON line; --out FILE also writes it):
  deal_search  bb_refill_values_pos at depth 3, value only, n boards x m deals, one launch: deal + search
  search       bb_plan_actions_pos at depth 3 (the parent's kernel; action and value, the action being required) over
               the same n * m (board, hand) pairs, the hands taken from the new call's own `hand` output and the
               replicas built outside the timed region: the search alone
  equal        both give the same values (a hand without a legal first move priced at the dead weight), checked
               before anything is timed
  deal_over_search  ratio of the medians; (deal_search - search) is what the dealing costs
The sets: mid-game boards (seeds 7 + i after 40 bb_rollout steps, as tools/bench_plan.py takes them).
Timing as tools/bench_plan.py: device events around back-to-back launches, warm-up first, `reps` repeats interleaved
between the two candidates in one process; median, minimum and maximum.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_plan import played, timed  # noqa: E402
from agents.greedy import DEFAULT_WEIGHTS  # noqa: E402
from runtime import kernels as K  # noqa: E402


def measure(board, combo, deals, seed, inner, reps, warmup):
    n, dev = board.numel(), board.device
    first = K.refill_values(board, DEFAULT_WEIGHTS, deals, seed, combo=combo, want=("hand", "value", "attempts"))
    rep_board = board.repeat_interleave(deals)
    rep_combo = combo.repeat_interleave(deals)
    rep_hand = first["hand"].reshape(-1).contiguous()
    new = {"value": torch.zeros((n, deals), dtype=torch.int64, device=dev)}
    action = torch.zeros(n * deals, dtype=torch.int32, device=dev)
    value = torch.zeros(n * deals, dtype=torch.int64, device=dev)

    def search():
        K.plan_actions(rep_board, rep_hand, DEFAULT_WEIGHTS, 3, combo=rep_combo, action=action, value=value)

    def deal_search():
        K.refill_values(board, DEFAULT_WEIGHTS, deals, seed, combo=combo, out=new)

    search()
    deal_search()
    lowest = torch.iinfo(torch.int64).min
    if not torch.equal(torch.where(value == lowest, DEFAULT_WEIGHTS["dead"], value), new["value"].reshape(-1)):
        sys.exit(f"bench_refill_values: the values differ on {n} boards")
    r = timed({"deal_search": deal_search, "search": search}, inner, reps, warmup)
    at = first["attempts"]
    return {"boards": n, "deals": deals, "equal": True, "first_draw_accepted": round(float((at == 1).double().mean()), 4),
            "max_attempts": int(at.abs().max()), "refused": int((at < 0).sum()), **r,
            "deal_over_search": round(r["deal_search"]["median_ms"] / r["search"]["median_ms"], 3),
            "deal_cost_ms": round(r["deal_search"]["median_ms"] - r["search"]["median_ms"], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, nargs="*", default=[512, 4096])
    ap.add_argument("--deals", type=int, default=16)
    ap.add_argument("--play", type=int, default=40, help="rollout steps played before the boards are taken")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--inner", type=int, default=5, help="launches per repeat")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_refill_values: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    out = {"played_steps": args.play, "inner": args.inner, "reps": args.reps, "depth": 3,
           "device": torch.cuda.get_device_name(0), "build_id": K.L.build_id()}
    for count in args.mid:
        env = played(count, args.play, dev)
        st = env.state()
        env.close()
        board = torch.from_numpy(st["board"].view(np.int64).copy()).to(dev)
        combo = torch.from_numpy(st["combo"].astype(np.int32)).to(dev)
        key = f"mid_{count}x{args.deals}"
        out[key] = measure(board, combo, args.deals, args.seed, args.inner, args.reps, args.warmup)
        print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
