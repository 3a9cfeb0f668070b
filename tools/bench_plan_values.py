#!/usr/bin/env python3
"""Diagnostics (not product): per-launch time of the per-action full-hand values (plan_values_kernel in
csrc/bb_lookahead.hip) on the positions of tools/bench_plan.py: N mid-game positions from a played-in rollout, a
bigger such set, and fresh boards, at depth 2 and 3.

Reported per position set and depth (one JSON line; --out FILE also writes it):
  values   bb_plan_values with all four outputs
  plan     bb_plan_actions with all four outputs (this build's plan_kernel), interleaved with values
  safe     bb_plan_values with the safe words alone (the evaluation path's call)
  chain    what the fused call replaces: bb_afterstates, a torch `nonzero` gather of the legal unfinished
           afterstates (a device-to-host sync), bb_plan_actions_pos at depth - 1 on the children, a scatter into
           q / rest / leaves.  It does not produce the safe words (a second child search under {"dead": -1} does;
           used only for the equality check).  Timed against `values` in a group of its own, one launch per repeat.
  values_over_plan, chain_over_values   ratios of the medians
  equal    q / rest / leaves (and safe) of the chain equal the fused call's, checked before anything is timed
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
from bench_lookahead import WEIGHTS, code_object_metadata  # noqa: E402
from bench_plan import INT64_MIN, Plan, played, timed, value_of  # noqa: E402
from runtime import kernels as K  # noqa: E402


class Chain:
    """q / rest / leaves [n, 192] built from the one-ply kernel and bb_plan_actions_pos on the children."""

    def __init__(self, env, w):
        self.env, self.w = env, w
        st = env.state()
        dev = env.device
        self.hand = torch.from_numpy(st["hand"].view("int32").copy()).to(dev)
        self.combo = torch.from_numpy(st["combo"].copy()).to(dev).long()

    def __call__(self, depth, weights=None, want_safe=False):
        env, n, dev = self.env, self.env.num_envs, self.env.device
        one = env.afterstates(out=K.afterstate_outputs(n, dev, want=("board", "score_gained", "aux")))
        f = K.unpack_aux(one["aux"])
        end = f["legal"] & (f["refill"] | f["dead"] | (depth == 1))
        q = torch.where(end, value_of(f, one["score_gained"], one["board"]), torch.full((n, 192), INT64_MIN, device=dev))
        rest = torch.where(end, 0xFFFF, -1).int()
        leaves = end.int()
        safe = end & ~f["dead"]
        root, act = torch.nonzero(f["legal"] & ~end, as_tuple=True)  # the gather: a device-to-host sync
        if root.numel():
            hand2 = (self.hand[root].long() | (torch.ones_like(act) << (18 + (act >> 6)))).int()
            combo2 = torch.where(f["lines"][root, act] > 0, self.combo[root] + 1, torch.zeros_like(root)).int()
            board2 = one["board"][root, act].contiguous()
            child = K.plan_actions(board2, hand2.contiguous(), self.w, depth - 1, combo=combo2.contiguous(),
                                   want_plan=True, want_leaves=True)
            moves1 = WEIGHTS["lines"] * f["lines"][root, act] + WEIGHTS["score"] * one["score_gained"][root, act].long()
            q[root, act] = moves1 + child["value"]
            rest[root, act] = (child["plan"][:, 0] & 0xFF) | ((child["plan"][:, 1] & 0xFF) << 8)
            leaves[root, act] = child["leaves"]
            if want_safe:
                alive = K.plan_actions(board2, hand2.contiguous(), {"dead": -1}, depth - 1, combo=combo2.contiguous())
                safe[root, act] = alive["value"] == 0
        return {"q": q, "rest": rest, "leaves": leaves, "safe": safe}


def measure(env, w, depths, inner, reps, warmup):
    n, dev = env.num_envs, env.device
    plan = Plan(env, w)
    chain = Chain(env, w)
    full = K.plan_value_outputs(n, dev)
    safe_only = {"safe": torch.zeros((n, 3), dtype=torch.int64, device=dev)}
    res = {"positions": n}
    for d in depths:
        env.plan_values(w, d, out=full)
        want = chain(d, want_safe=True)
        equal = {k: bool(torch.equal(full[k], want[k])) for k in ("q", "rest", "leaves")}
        equal["safe"] = bool(torch.equal(K.mask_bits_to_bool(full["safe"]), want["safe"]))
        env.plan_values(w, d, out=safe_only)
        equal["safe_alone"] = bool(torch.equal(safe_only["safe"], full["safe"]))
        r = timed({"values": lambda: env.plan_values(w, d, out=full), "plan": lambda: plan(d),
                   "safe": lambda: env.plan_values(w, d, out=safe_only)}, inner, reps, warmup)
        c = timed({"values": lambda: env.plan_values(w, d, out=full), "chain": lambda: chain(d)}, 1, reps, 1)
        res[f"d{d}"] = {"equal": equal, "values": r["values"], "plan": r["plan"], "safe": r["safe"],
                        "chain": c["chain"], "values_single_launch": c["values"],
                        "values_over_plan": round(r["values"]["median_ms"] / r["plan"]["median_ms"], 3),
                        "safe_over_values": round(r["safe"]["median_ms"] / r["values"]["median_ms"], 3),
                        "chain_over_values": round(c["chain"]["median_ms"] / c["values"]["median_ms"], 2),
                        "leaves": int(full["leaves"].long().sum())}
    return res


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
        sys.exit("bench_plan_values: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    w = K.L.greedy_weights(WEIGHTS)
    out = {"played_steps": args.play, "inner": args.inner, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "build_id": K.L.build_id()}
    for key, count, steps, inner in (("mid", args.positions, args.play, args.inner),
                                     ("mid_big", args.big, args.play, max(1, args.inner // 5)),
                                     ("fresh", args.fresh, 0, max(1, args.inner // 5))):
        if count:
            env = played(count, steps, dev)
            out[key] = measure(env, w, (2, 3), inner, args.reps, args.warmup)
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
