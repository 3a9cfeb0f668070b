#!/usr/bin/env python3
"""Policy distillation timings on one MI355X ("policy distillation").

(1) The loss: one ``bb_distill_loss_fused`` launch against ``agents.ppo.distill_loss_torch`` forward + backward
    (the torch-op chain it replaces, same build, same inputs) at B = 2,048 and 65,536, f32 and bf16 logits.  The
    candidates are interleaved in one process; every repeat is timed by device events around ``--calls`` calls;
    the median (min - max) of ``--repeats`` repeats is reported per call.  The bar: on every shape the slowest
    repeat of the fused call is below the fastest repeat of the torch chain.
(2) Reported, not gated: ``bb_plan_values_pos`` (q only) on a minibatch of 2,048 stored positions at depth 2 and 3,
    and the whole distill step (search at ``--depth``, forward, fused loss, backward, clip + Adam; eager) on that
    minibatch.  tools/bench_ppo.py gives the PPO step beside it.

Inputs of (1): ~25% of the actions legal per row, q uniform in [-400, 400) on them and INT64_MIN elsewhere, normal
logits; tau = 50.  Positions of (2): a 2,048-env rollout under the hand-safe mask, 24 steps in.

Writes one JSON object to --out (if given) and prints it as one line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"), REPO]

import torch  # noqa: E402


def timed(fn, calls, repeats, warmup):
    """Per-call milliseconds of ``repeats`` device-event windows of ``calls`` calls each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def interleaved(fns, calls, repeats, warmup):
    """{name: [ms per call] * repeats}, one repeat of every candidate in turn."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            res[k] += timed(fn, calls, 1, 0)
    return res


def summary(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2),
            "max_us": round(max(ms) * 1e3, 2), "repeats": len(ms)}


def loss_inputs(B, bf16, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    legal = torch.rand((B, 192), device=dev, generator=g) < 0.25
    legal[:, 0] = True
    q = torch.randint(-400, 400, (B, 192), device=dev, generator=g, dtype=torch.int64)
    q = torch.where(legal, q, torch.full_like(q, torch.iinfo(torch.int64).min))
    from runtime import kernels as K

    mb = K.pack_mask(legal)
    x = torch.randn((B, 192), device=dev, generator=g) * 2.0
    return (x.bfloat16() if bf16 else x), mb, q


def bench_loss(B, bf16, tau, args, dev):
    from agents.ppo import distill_loss_torch
    from runtime import kernels as K
    from runtime import lib as L

    lib = L.load()
    x, mb, q = loss_inputs(B, bf16, dev)
    seed = torch.ones(1, dtype=torch.float32, device=dev)
    ws = torch.empty((lib.bb_distill_loss_workspace_bytes(B) + 7) // 8, dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.empty(6, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dl = torch.empty_like(x)
    a = L.DistillLossArgs(logits=x.data_ptr(), bf16=int(bf16), mask_bits=mb.data_ptr(), q=q.data_ptr(), B=B, tau=tau,
                          grad_loss=seed.data_ptr(), dlogits=dl.data_ptr(), ws=ws.data_ptr(), cnt=cnt.data_ptr(),
                          stats=stats.data_ptr(), loss=loss.data_ptr())
    stream = K._s(dev)

    def fused():
        L.check(lib.bb_distill_loss_fused(C.byref(a), stream), "bb_distill_loss_fused")

    xt = x.clone().requires_grad_(True)

    def chain():
        xt.grad = None
        l, _ = distill_loss_torch(xt, mb, q, tau)
        l.backward()

    res = interleaved({"fused": fused, "torch": chain}, args.calls, args.repeats, args.warmup)
    fused()
    chain()
    torch.cuda.synchronize()
    ref_l, ref_s = distill_loss_torch(x, mb, q, tau)
    out = {"B": B, "logits": "bf16" if bf16 else "f32", "tau": tau, "fused": summary(res["fused"]),
           "torch_chain": summary(res["torch"]),
           "bar_met": max(res["fused"]) < min(res["torch"]),
           "loss_fused": float(loss[0]), "loss_torch": float(ref_l),
           "max_abs_dlogits_diff": float((dl.float() - xt.grad.float()).abs().max())}
    out["speedup_median"] = round(out["torch_chain"]["median_us"] / out["fused"]["median_us"], 1)
    return out


def bench_training(args, dev):
    from agents import PPOAgent, PPOConfig
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K
    from training.trainer import DeviceRollout

    torch.manual_seed(0)
    agent = PPOAgent(PPOConfig(batch_size=2048), device=dev, sample_seed=1)
    if args.autocast == "bf16":
        agent.autocast_dtype = torch.bfloat16
    agent.train()
    n, T = 2048, 8
    roll = DeviceRollout(n, 0, n, 42, {}, T, dev, safe_mask=True, positions=True)
    roll.reset()
    for _ in range(3):
        roll.collect(agent)
    x, mb, board, hand, combo = next(roll.buffer.get_position_minibatches(2048))
    q = torch.empty((2048, 192), dtype=torch.int64, device=dev)
    w = K._weights(DEFAULT_WEIGHTS)
    out = {"positions": "2,048 of a 2,048-env x 8-step rollout under the hand-safe mask, 16 steps in",
           "compute_dtype": "bf16 autocast" if args.autocast == "bf16" else "fp32"}
    searches = {f"depth{d}": (lambda d=d: K.plan_values(board, hand, w, d, combo=combo, out={"q": q}))
                for d in (2, 3)}
    res = interleaved(searches, args.search_calls, args.repeats, 2)
    for k, ms in res.items():
        out[f"plan_values_pos_{k}"] = summary(ms)

    def step():
        K.plan_values(board, hand, w, args.depth, combo=combo, out={"q": q})
        agent.distill_minibatch(x, mb, q, 50.0)

    def step_no_search():
        agent.distill_minibatch(x, mb, q, 50.0)

    res = interleaved({"distill_step": step, "distill_step_without_search": step_no_search}, args.step_calls,
                      args.repeats, 3)
    out["distill_step_depth"] = args.depth
    for k, ms in res.items():
        out[k] = summary(ms)
    roll.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="loss calls per timed window")
    ap.add_argument("--search-calls", type=int, default=5)
    ap.add_argument("--step-calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--autocast", choices=["none", "bf16"], default="none")
    ap.add_argument("--skip-training", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py measures on the HIP device: none is visible")
    dev = torch.device("cuda", 0)
    from runtime import lib as L

    result = {"workload": "policy distillation: fused loss vs torch chain, search and step per 2,048 positions",
              "device": torch.cuda.get_device_name(dev), "build_id": L.build_id(),
              "loss": [bench_loss(B, bf16, 50.0, args, dev) for B in (2048, 65536) for bf16 in (False, True)]}
    result["bar_met_on_every_shape"] = all(r["bar_met"] for r in result["loss"])
    if not args.skip_training:
        result["training"] = bench_training(args, dev)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
