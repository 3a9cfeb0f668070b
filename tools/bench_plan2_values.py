#!/usr/bin/env python3
"""Time the two-hand decision as one call (bb_plan2_values) against the chain of kernels the two-hand agent runs.

The protocol of tools/bench_values_ext.py: mid-game roots (seeds 7 + i after 40 steps of random legal play), depth 3,
8 candidates x 16 deals, one process, device events, a warm-up, the variants interleaved round by round.

  call against chain   `chain` is what ``TwoHandShapeAgent`` launches for the same work, all on existing kernels:
                       bb_plan_values_ext_pos (q, rest) + bb_play_plan_pos (the n x K plans) + bb_refill_values_ext_pos
                       (the refill leaves).  The plans and the compacted refill leaves are made before the timed region
                       and none of the agent's torch steps is timed: that favours the yardstick.  `plan2` is
                       bb_plan2_values_pos with the action alone asked for, into a workspace made once.  The actions are
                       checked equal to the agent's before anything is timed.  Gate: the call's median is no more than the
                       chain's median plus the chain's own min-max spread.
  agent                moves per second of ``PopulationTwoHandAgent`` (equal rows) against ``TwoHandShapeAgent`` /
                       ``TwoHandPlanAgent`` on the same games, wall clock with a device sync at the end of a game,
                       alternating, a warm-up game first.  Gate: not slower beyond the old agent's own spread.

Both under the default weights and under config/plan_d3_shape_tuned.json.  Prints one JSON line and writes it to
--output.

    python tools/bench_plan2_values.py --output profiles/plan2_values/bench_run1.json
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd")
sys.path[:0] = [PKG, REPO, os.path.join(REPO, "tools")]

import torch  # noqa: E402
from bench_values_ext import mid_game, summary, timed  # noqa: E402


def chain_and_call(n, weights, k, deals, depth, dev, warmup, rounds):
    from agents.greedy import TwoHandPlanAgent, two_hand_agent_class
    from runtime import kernels as K

    board, hand, combo = mid_game(n, 40, 7, dev)
    rows = K.eval_rows(weights, device=dev)
    agent = two_hand_agent_class(weights)(weights, depth=depth, candidates=k, deals=deals, seed=3, device=dev)
    seed = TwoHandPlanAgent.deal_seed(3, 0)
    # the chain's inputs, made outside the timed region as the agent's torch steps make them
    pv = {"q": torch.empty((n, 192), dtype=torch.int64, device=dev),
          "rest": torch.empty((n, 192), dtype=torch.int32, device=dev)}
    K.plan_values_ext(board, hand, rows, depth, combo=combo, out=pv)
    want = agent._decide(board, hand, combo, pv["q"], pv["rest"])
    cand = torch.sort(pv["q"], dim=1, descending=True, stable=True).indices[:, :k]
    valid = pv["q"].gather(1, cand) != torch.iinfo(torch.int64).min
    a2, a3 = K.unpack_rest(pv["rest"].gather(1, cand))
    plan = torch.stack([cand.to(torch.int32), a2.to(torch.int32), a3.to(torch.int32)], dim=2)
    plan = torch.where(valid.unsqueeze(2), plan, torch.full_like(plan, -1)).view(n * k, 3).contiguous()
    rb, rh, rc = board.repeat_interleave(k), hand.repeat_interleave(k), combo.repeat_interleave(k)
    leaf = {key: torch.empty(n * k, dtype=K.PLAY_PLAN_OUTPUTS[key], device=dev)
            for key in ("board", "combo", "lines", "score", "status")}
    K.play_plan(rb, rh, plan, rc, out=leaf)
    idx = torch.nonzero(((leaf["status"] & K.PLAY_REFILL) != 0) & valid.view(-1)).view(-1)
    lb, lc = leaf["board"][idx].contiguous(), leaf["combo"][idx].contiguous()
    root = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(k)[idx].contiguous()
    rv = {"value": torch.empty((idx.numel(), deals), dtype=torch.int64, device=dev)}

    def chain():
        K.plan_values_ext(board, hand, rows, depth, combo=combo, out=pv)
        K.play_plan(rb, rh, plan, rc, out=leaf)
        K.refill_values_ext(lb, rows, deals, seed, combo=lc, stream=root, depth=depth, out=rv)

    work = torch.empty(K.plan2_work_bytes(n, k, deals), dtype=torch.uint8, device=dev)
    out = {"action": torch.empty(n, dtype=torch.int32, device=dev)}

    def plan2():
        K.plan2_values(board, hand, rows, k, deals, seed, combo=combo, depth=depth, out=out, work=work)

    plan2()
    torch.cuda.synchronize()
    if not torch.equal(out["action"].long(), want):
        raise SystemExit(f"bb_plan2_values and the agent's chain disagree at {n} roots")
    ms = {"chain": [], "plan2": []}
    for rnd in range(warmup + rounds):
        for name, fn in (("chain", chain), ("plan2", plan2)):
            t = timed(fn)
            if rnd >= warmup:
                ms[name].append(t)
    res = {name: summary(v) for name, v in ms.items()}
    spread = res["chain"]["max_ms"] - res["chain"]["min_ms"]
    res["ratio_plan2_to_chain"] = res["plan2"]["median_ms"] / res["chain"]["median_ms"]
    res["gate_ms"] = res["chain"]["median_ms"] + spread
    res["gate_met"] = res["plan2"]["median_ms"] <= res["gate_ms"]
    res["refill_leaves"], res["candidates_present"] = int(idx.numel()), int(valid.sum())
    return res


def game(agent, n, moves, dev):
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(n, [42 + i for i in range(n)], device=dev)
    env.reset()
    act = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(moves):
        agent.act_env(env, act)
        env.step(act)
    env.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    env.close()
    return n * moves / dt


def agents(n, moves, weights, k, deals, depth, dev, repeats):
    from agents.greedy import PopulationTwoHandAgent, two_hand_agent_class
    from runtime import kernels as K

    def old():
        return two_hand_agent_class(weights)(weights, depth=depth, candidates=k, deals=deals, seed=3, device=dev)

    def new():
        return PopulationTwoHandAgent(K.eval_rows(weights, device=dev), depth=depth, candidates=k, deals=deals, seed=3,
                                      device=dev)

    game(old(), n, max(moves // 10, 5), dev)  # warm-up games
    game(new(), n, max(moves // 10, 5), dev)
    rate = {"two_hand_agent": [], "population_agent": []}
    for _ in range(repeats):
        rate["two_hand_agent"].append(game(old(), n, moves, dev))
        rate["population_agent"].append(game(new(), n, moves, dev))
    res = {name: {"median_moves_per_s": statistics.median(v), "min": min(v), "max": max(v), "games": len(v)}
           for name, v in rate.items()}
    o, p = res["two_hand_agent"], res["population_agent"]
    res["ratio_population_to_two_hand"] = p["median_moves_per_s"] / o["median_moves_per_s"]
    res["gate_met"] = p["median_moves_per_s"] >= o["median_moves_per_s"] - (o["max"] - o["min"])
    return res


def main():
    from agents.greedy import DEFAULT_WEIGHTS
    from runtime import lib as L

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--deals", type=int, default=16)
    ap.add_argument("--output", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with open(os.path.join(PKG, "config", "plan_d3_shape_tuned.json")) as f:
        tuned = json.load(f)["weights"]
    sets = {"default": dict(DEFAULT_WEIGHTS), "shape_tuned": tuned}
    k, deals = args.candidates, args.deals
    rec = {"record": "bench_plan2_values", "depth": 3, "candidates": k, "deals": deals, "build_id": L.build_id(),
           "device": torch.cuda.get_device_name(0), "call": {}, "agent": {}}
    for name, w in sets.items():
        for n in (32, 512):
            rec["call"][f"{name}/{n}"] = chain_and_call(n, w, k, deals, 3, dev, args.warmup, args.rounds)
    for n, moves in ((32, 600), (512, 100)):
        rec["agent"][f"shape_tuned/{n}x{moves}"] = agents(n, moves, tuned, k, deals, 3, dev, args.repeats)
    line = json.dumps(rec)
    print(line)
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
