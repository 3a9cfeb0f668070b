#!/usr/bin/env python3
"""Search-guided PPO timings on one MI355X ("search-guided PPO").

(1) The loss: one ``bb_guided_loss_fused`` launch against what a caller would run without it -- ``bb_ppo_loss_fused``
    plus ``bb_distill_loss_fused`` plus the add of the two ``dlogits`` -- on the same build and the same inputs, at
    B = 2,048 and 65,536, f32 and bf16 logits / values.  Expanding the f32 mask the PPO kernel reads is left out of
    the pair's time, which favours the pair.  The candidates are interleaved in one process; every repeat is timed by
    device events around ``--calls`` calls; the median (min - max) of ``--repeats`` repeats is reported per call.  The
    bar: on every shape the slowest repeat of the fused call is below the fastest repeat of the pair.
(2) Reported, not gated: the captured guided step (``PPOAgent.guided_minibatch``) on a minibatch of 2,048 stored
    positions beside the captured PPO step (``train_minibatch``) and the eager distill step (``distill_minibatch``)
    on the same minibatch, all without the search; ``--autocast bf16`` for the bf16 network.

Inputs of (1): ~25% of the actions legal per row, q uniform in [-400, 400) on them and INT64_MIN elsewhere, normal
logits, actions inside the mask, old log-probs within 0.3 of the current ones; tau = 50, coefficients (1, 0.5, 0.01,
0.5).  Positions of (2): a 2,048-env x 8-step rollout under the hand-safe mask, 16 steps in.

Writes one JSON object to --out (if given) and prints it as one line.
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd"), REPO,
                os.path.dirname(os.path.abspath(__file__))]

import torch  # noqa: E402

from bench_distill import interleaved, loss_inputs, summary  # noqa: E402

CLIP, COEFS, TAU = 0.2, (1.0, 0.5, 0.01, 0.5), 50.0


def bench_loss(B, bf16, args, dev):
    from runtime import kernels as K
    from runtime import lib as L

    lib = L.load()
    x, mb, q = loss_inputs(B, bf16, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    maskf = K.mask_bits_to_bool(mb).float().contiguous()
    actions = torch.multinomial(maskf, 1, generator=g).squeeze(1)
    with torch.no_grad():
        logp = torch.log_softmax(x.float().masked_fill(maskf == 0, float("-inf")), dim=-1)
        old = logp.gather(1, actions[:, None]).squeeze(1) + (torch.rand(B, device=dev, generator=g) - 0.5) * 0.6
    adv = torch.randn(B, device=dev, generator=g)
    ret = torch.randn(B, device=dev, generator=g)
    v = torch.randn(B, device=dev, generator=g)
    v = v.bfloat16() if bf16 else v
    seed = torch.ones(1, dtype=torch.float32, device=dev)
    stream = K._s(dev)

    def outs(nbytes, nstats):
        return dict(ws=torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev),
                    cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                    stats=torch.empty(nstats, dtype=torch.float32, device=dev),
                    loss=torch.empty(1, dtype=torch.float32, device=dev))

    ptr = lambda d: {k: t.data_ptr() for k, t in d.items()}  # noqa: E731
    go, po, do = (outs(lib.bb_guided_loss_workspace_bytes(B), 12), outs(lib.bb_ppo_loss_workspace_bytes(B), 6),
                  outs(lib.bb_distill_loss_workspace_bytes(B), 6))
    gdl, gdv = torch.empty_like(x), torch.empty_like(v)
    pdl, pdv, ddl = torch.empty_like(x), torch.empty_like(v), torch.empty_like(x)
    rows = dict(actions=actions.data_ptr(), old_logp=old.data_ptr(), adv=adv.data_ptr(), ret=ret.data_ptr())
    ga = L.GuidedLossArgs(logits=x.data_ptr(), values=v.data_ptr(), bf16=int(bf16), mask_bits=mb.data_ptr(),
                          q=q.data_ptr(), B=B, clip=CLIP, policy_coef=COEFS[0], value_coef=COEFS[1],
                          entropy_coef=COEFS[2], distill_coef=COEFS[3], tau=TAU, grad_loss=seed.data_ptr(),
                          dlogits=gdl.data_ptr(), dvalues=gdv.data_ptr(), **rows, **ptr(go))
    pa = L.PpoLossArgs(logits=x.data_ptr(), values=v.data_ptr(), bf16=int(bf16), mask=maskf.data_ptr(), B=B, clip=CLIP,
                       value_coef=COEFS[1], entropy_coef=COEFS[2], grad_loss=seed.data_ptr(), dlogits=pdl.data_ptr(),
                       dvalues=pdv.data_ptr(), **rows, **ptr(po))
    beta = torch.full((1,), COEFS[3], dtype=torch.float32, device=dev)  # the pair's distillation seed: beta * 1
    da = L.DistillLossArgs(logits=x.data_ptr(), bf16=int(bf16), mask_bits=mb.data_ptr(), q=q.data_ptr(), B=B, tau=TAU,
                           grad_loss=beta.data_ptr(), dlogits=ddl.data_ptr(), **ptr(do))

    def fused():
        L.check(lib.bb_guided_loss_fused(C.byref(ga), stream), "bb_guided_loss_fused")

    def pair():
        L.check(lib.bb_ppo_loss_fused(C.byref(pa), stream), "bb_ppo_loss_fused")
        L.check(lib.bb_distill_loss_fused(C.byref(da), stream), "bb_distill_loss_fused")
        pdl.add_(ddl)

    res = interleaved({"fused": fused, "pair": pair}, args.calls, args.repeats, args.warmup)
    fused()
    pair()
    torch.cuda.synchronize()
    total_pair = float(po["loss"][0]) + COEFS[3] * float(do["loss"][0])
    out = {"B": B, "logits": "bf16" if bf16 else "f32", "fused": summary(res["fused"]),
           "ppo_plus_distill_plus_add": summary(res["pair"]), "bar_met": max(res["fused"]) < min(res["pair"]),
           "loss_fused": float(go["loss"][0]), "loss_pair": total_pair,
           "max_abs_dlogits_diff": float((gdl.float() - pdl.float()).abs().max()),
           "max_abs_dvalues_diff": float((gdv.float() - pdv.float()).abs().max())}
    out["speedup_median"] = round(out["ppo_plus_distill_plus_add"]["median_us"] / out["fused"]["median_us"], 2)
    return out


def bench_training(args, dev):
    from agents import PPOAgent, PPOConfig
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import kernels as K
    from training.trainer import DeviceRollout

    def agent():
        torch.manual_seed(0)
        a = PPOAgent(PPOConfig(batch_size=2048), device=dev, sample_seed=1)
        if args.autocast == "bf16":
            a.autocast_dtype = torch.bfloat16
        a.train()
        return a

    guided, ppo, distill = agent(), agent(), agent()
    n, T = 2048, 8
    roll = DeviceRollout(n, 0, n, 42, {}, T, dev, safe_mask=True, positions=True)
    roll.reset()
    for _ in range(3):
        roll.collect(guided)
    roll.buffer.compute_returns_and_advantages(guided.values_device(roll.x), 0.99, 0.95)
    x, mb, a, lp, adv, ret, board, hand, combo = next(roll.buffer.get_guided_minibatches(2048))
    q = K.plan_values(board, hand, K._weights(DEFAULT_WEIGHTS), 2, combo=combo, want=("q",))["q"]
    maskf = K.mask_bits_to_bool(mb).float().contiguous()
    coefs = (*COEFS, TAU)
    steps = {"guided_step_captured": lambda: guided.guided_minibatch(x, mb, a, lp, adv, ret, q, coefs),
             "ppo_step_captured": lambda: ppo.train_minibatch(x, maskf, a, lp, adv, ret),
             "distill_step_eager": lambda: distill.distill_minibatch(x, mb, q, TAU)}
    res = interleaved(steps, args.step_calls, args.repeats, 3)
    out = {"positions": "2,048 of a 2,048-env x 8-step rollout under the hand-safe mask, 16 steps in; no search",
           "compute_dtype": "bf16 autocast" if args.autocast == "bf16" else "fp32"}
    for k, ms in res.items():
        out[k] = summary(ms)
    roll.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="loss calls per timed window")
    ap.add_argument("--step-calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--autocast", choices=["none", "bf16"], default="none")
    ap.add_argument("--skip-training", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided.py measures on the HIP device: none is visible")
    dev = torch.device("cuda", 0)
    from runtime import lib as L

    result = {"workload": "search-guided PPO: fused loss vs bb_ppo_loss_fused + bb_distill_loss_fused + add; steps",
              "device": torch.cuda.get_device_name(dev), "build_id": L.build_id(),
              "loss": [bench_loss(B, bf16, args, dev) for B in (2048, 65536) for bf16 in (False, True)]}
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
