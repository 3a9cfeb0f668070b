#!/usr/bin/env python3
"""Diagnostics (not product): per-launch time of the full-hand lookahead (plan_kernel in csrc/bb_lookahead.hip) at
N positions taken from a played-in rollout, and on fresh boards.

Reported (one JSON line; --out FILE also writes it):
  plan_d1 / plan_d2 / plan_d3   bb_plan_actions (all four outputs) at depth 1, 2, 3: ms per launch, the leaves of
                                the launch (sum of the `leaves` output) and leaves per second
  greedy                        bb_greedy_actions on the same positions, interleaved with plan_d1
  chain_d2                      what the fused depth-2 search replaces: bb_afterstates, a torch gather of the legal
                                unfinished afterstates, bb_afterstates_pos on them, torch reductions to the best
                                value per position (the plan itself is not even recovered)
  plan_d3_big                   depth 3 at --big positions (0: skipped)
  fresh_d3                      depth 3 on --fresh freshly reset boards (0: skipped)
  host_d3                       the host backend (csrc/bb_host.cpp) on the same N positions at depth 3, wall clock
  regs                          VGPRs / SGPRs / LDS / scratch of the kernels from the code object's metadata
Timing: device events around `inner` back-to-back launches, warm-up first, `reps` repeats interleaved between the
candidates in one process; the median, minimum and maximum of the repeats are reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lookahead import FIELDS, WEIGHTS, code_object_metadata  # noqa: E402
from runtime import kernels as K  # noqa: E402
from runtime.device_env import DeviceEnvBatch  # noqa: E402

INT64_MIN = -(2 ** 63)


def timed(fns, inner, reps, warmup):
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
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
            for k, v in times.items()}


def played(n, steps, dev):
    env = DeviceEnvBatch(n, [7 + i for i in range(n)], device=dev)
    env.reset()
    if steps:
        mb = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        a0 = torch.zeros(n, dtype=torch.int32, device=dev)
        env.obs(mask_bits=mb)
        env.random_actions(mb, a0, step=0)
        env.rollout(steps, a0, torch.zeros((steps, n), device=dev), torch.zeros((steps, n), dtype=torch.uint8, device=dev))
    env.sync()
    return env


class Plan:
    def __init__(self, env, w):
        n, dev = env.num_envs, env.device
        self.env, self.w = env, w
        self.act = torch.zeros(n, dtype=torch.int32, device=dev)
        self.val = torch.zeros(n, dtype=torch.int64, device=dev)
        self.plan = torch.zeros((n, 3), dtype=torch.int32, device=dev)
        self.leaves = torch.zeros(n, dtype=torch.int32, device=dev)

    def __call__(self, depth):
        self.env.plan_actions(self.act, self.w, depth, value=self.val, plan=self.plan, leaves=self.leaves)

    def total_leaves(self, depth):
        self(depth)
        return int(self.leaves.long().sum())


def with_rate(t, leaves):
    t = dict(t)
    t["leaves"] = leaves
    t["leaves_per_s"] = round(leaves / (t["median_ms"] * 1e-3))
    return t


def value_of(f, score, board):
    b = board - ((board >> 1) & 0x5555555555555555)  # popcount of the board bits
    b = (b & 0x3333333333333333) + ((b >> 2) & 0x3333333333333333)
    b = (b + (b >> 4)) & 0x0F0F0F0F0F0F0F0F
    f = dict(f, score=score.long(), filled=((b * 0x0101010101010101) >> 56) & 0xFF)
    return sum(WEIGHTS[k] * f[k].long() for k in FIELDS if WEIGHTS[k])


def chain_depth2(env, st):
    """The depth-2 search value built from the one-ply kernels and torch."""
    one = env.afterstates(out=K.afterstate_outputs(env.num_envs, env.device, want=("board", "score_gained", "aux")))
    f = K.unpack_aux(one["aux"])
    v1 = value_of(f, one["score_gained"], one["board"])
    end = f["legal"] & (f["refill"] | f["dead"])
    best = torch.where(end, v1, torch.full_like(v1, INT64_MIN)).max(dim=1).values
    root, act = torch.nonzero(f["legal"] & ~end, as_tuple=True)  # the gather: a device-to-host sync
    hand2 = (st["hand"][root].long() | (torch.ones_like(act) << (18 + (act >> 6)))).int()
    combo2 = torch.where(f["lines"][root, act] > 0, st["combo"][root] + 1, torch.zeros_like(root)).int()
    two = K.afterstates(one["board"][root, act].contiguous(), hand2.contiguous(), combo2.contiguous(),
                        out=K.afterstate_outputs(root.numel(), env.device, want=("board", "score_gained", "aux")))
    f2 = K.unpack_aux(two["aux"])
    moves1 = (WEIGHTS["lines"] * f["lines"][root, act] + WEIGHTS["score"] * one["score_gained"][root, act].long())
    v2 = value_of(f2, two["score_gained"], two["board"]) + moves1[:, None]
    v2 = torch.where(f2["legal"], v2, torch.full_like(v2, INT64_MIN)).max(dim=1).values
    return best.scatter_reduce(0, root, v2, "amax")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--fresh", type=int, default=4096)
    ap.add_argument("--play", type=int, default=40, help="rollout steps played before the positions are taken")
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3, help="0: no host-backend timing")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plan: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    n = args.positions
    w = K.L.greedy_weights(WEIGHTS)
    env = played(n, args.play, dev)
    plan = Plan(env, w)
    host_state = env.state()
    st = {"hand": torch.from_numpy(host_state["hand"].view("int32").copy()).to(dev),
          "combo": torch.from_numpy(host_state["combo"].copy()).to(dev).long()}
    gact = torch.zeros(n, dtype=torch.int32, device=dev)
    gval = torch.zeros(n, dtype=torch.int64, device=dev)

    leaves = {d: plan.total_leaves(d) for d in (1, 2, 3)}
    # before anything is timed: depth 1 is the greedy kernel's answer, the chain finds the fused depth-2 value
    env.greedy_actions(gact, w, value=gval)
    plan(1)
    d1_equal = bool(torch.equal(plan.act, gact) and torch.equal(plan.val, gval))
    plan(2)
    chain_equal = bool(torch.equal(chain_depth2(env, st), plan.val))

    out = {"positions": n, "played_steps": args.play, "inner": args.inner, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "build_id": K.L.build_id(),
           "depth1_equals_greedy": d1_equal, "chain_value_equals_fused": chain_equal}
    r = timed({"plan_d1": lambda: plan(1), "greedy": lambda: env.greedy_actions(gact, w, value=gval)},
              args.inner * 5, args.reps, args.warmup)
    out["plan_d1"], out["greedy"] = with_rate(r["plan_d1"], leaves[1]), r["greedy"]
    out["plan_d1_over_greedy"] = round(r["plan_d1"]["median_ms"] / r["greedy"]["median_ms"], 3)
    r = timed({"plan_d2": lambda: plan(2), "chain_d2": lambda: chain_depth2(env, st)}, args.inner, args.reps,
              args.warmup)
    out["plan_d2"], out["chain_d2"] = with_rate(r["plan_d2"], leaves[2]), r["chain_d2"]
    out["fused_d2_speedup_over_chain"] = round(r["chain_d2"]["median_ms"] / r["plan_d2"]["median_ms"], 2)
    r = timed({"plan_d3": lambda: plan(3)}, args.inner, args.reps, args.warmup)
    out["plan_d3"] = with_rate(r["plan_d3"], leaves[3])

    if args.host_reps:
        from runtime.build import build_host_lib

        build_host_lib(verbose=False)
        hb = torch.from_numpy(host_state["board"].view("int64").copy())
        hh = torch.from_numpy(host_state["hand"].view("int32").copy())
        hc = torch.from_numpy(host_state["combo"].copy())
        ts = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            res = K.plan_actions(hb, hh, w, 3, combo=hc, want_plan=True, want_leaves=True)
            ts.append((time.perf_counter() - t0) * 1e3)
        plan(3)
        out["host_d3"] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                          "max_ms": round(max(ts), 3), "threads": torch.get_num_threads(),
                          "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
                          "equals_hip": bool(torch.equal(res["value"], plan.val.cpu())
                                             and torch.equal(res["plan"], plan.plan.cpu())
                                             and torch.equal(res["leaves"], plan.leaves.cpu()))}
        out["host_d3"]["leaves_per_s"] = round(leaves[3] / (out["host_d3"]["median_ms"] * 1e-3))
    env.close()

    for key, count, steps in (("plan_d3_big", args.big, args.play), ("fresh_d3", args.fresh, 0)):
        if count:
            e = played(count, steps, dev)
            p = Plan(e, w)
            total = p.total_leaves(3)
            r = timed({key: lambda: p(3)}, max(1, args.inner // 5), args.reps, 1)
            out[key] = with_rate(r[key], total)
            out[key]["positions"] = count
            e.close()
    out["regs"] = code_object_metadata()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
