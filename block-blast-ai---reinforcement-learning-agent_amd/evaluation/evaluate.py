"""Evaluation of a trained agent (reference scripts/evaluate.py:23-90 and its
CLI 119-184).

The reference plays ``num_episodes`` games one after another on a single
``BlockBlastEnv`` re-seeded ``seed + episode``.  Episodes are independent, so
here they run side by side: one device env per episode (seeded
``seed + episode``, no auto-reset) stepped in lockstep, the policy evaluated
for all unfinished games in one forward pass, each game's statistics latched
at its termination.  With ``deterministic=True`` (argmax) and the agent in
eval mode this gives the same per-episode results as the sequential loop.
``render=True`` uses the sequential single-env path so games can be shown.

Beyond the reference: ``--agent greedy`` / ``--agent plan`` / ``--agent random`` evaluate the untrained baselines of
``agents/greedy.py`` on the same seeds (no checkpoint needed), so a checkpoint's scores have something to be
compared with.  An agent with ``act_env(env_batch, out)`` picks its actions from the device env itself (the
fused one-ply kernel); every other agent goes through ``act_device`` as before.

``--agent plan2`` is ``TwoHandPlanAgent``: the full-hand search with a sampled look past the refill
(``--candidates`` first moves, ``--deals`` dealt next hands each, ``bb_refill_values``; both defaults are untuned).
``--agent playout`` is ``PlayoutPlanAgent``: the same with every deal carried on for ``--hands`` hands
(``bb_playout_values``: deal, search, play the plan, deal again; the default 2 is untuned).

``--safe-mask`` (off by default) restricts the policy to hand-safe actions: the legal moves after which the rest of
the hand can still be placed in some order (``bb_plan_values``' safe words, from ``bb_safe_mask``: one more launch per move).  For
``--agent ppo`` they are AND-ed into the mask the policy samples under, for ``--agent random`` the agent draws from
them; a position without a safe move keeps its legal mask.

``--census`` (off by default) prices every refill: after each move that leaves an unfinished game with a whole new
hand, ``bb_refill_census`` counts on the board as it stands how many of the 37^3 hands the dealer could have
accepted, and the result gains, per episode and as means, the expected number of lost deals, the survival
probability, the lowest and the mean solvable fraction and the number of refills (``census_summary``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Any, Dict

import numpy as np
import torch


def _summary(scores, lengths, lines, combos) -> Dict[str, Any]:
    return {
        "num_episodes": len(scores), "mean_score": np.mean(scores), "std_score": np.std(scores),
        "min_score": np.min(scores), "max_score": np.max(scores), "median_score": np.median(scores),
        "mean_length": np.mean(lengths), "std_length": np.std(lengths),
        "mean_lines_cleared": np.mean(lines), "mean_max_combo": np.mean(combos),
        "scores": list(scores), "lengths": list(lengths),
    }


CENSUS_KEYS = ("expected_losses", "survival", "min_solvable_fraction", "mean_solvable_fraction", "refills")


def census_summary(counts: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The per-episode census figures from the counts of every refill: counts int64 [R, n] on the CPU, row r the
    census count of each game's board at its r-th refill step and -1 where that game had no refill then (finished).
    With hazard = ``refill_hazard(count)`` and fraction = count / 37^3 over a game's refills: expected_losses = sum
    of hazard, survival = product of (1 - hazard), min_solvable_fraction, mean_solvable_fraction (both 1.0 for a
    game without a refill), float64 [n] each, and refills int64 [n].  Computed on the host from the integer counts,
    so both backends give the same floats."""
    from runtime.kernels import NUM_HANDS, refill_hazard

    counts = counts.to(torch.int64).cpu()
    n = counts.shape[1]
    m = counts >= 0
    c = counts.clamp(min=0)
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    hz = torch.where(m, refill_hazard(c), zero)
    frac = torch.where(m, c.double() / NUM_HANDS, one)
    refills = m.sum(dim=0)
    lowest = frac.min(dim=0).values if counts.shape[0] else torch.ones(n, dtype=torch.float64)
    mean = torch.where(refills > 0, torch.where(m, frac, zero).sum(dim=0) / refills.clamp(min=1).double(), one)
    return {"expected_losses": hz.sum(dim=0), "survival": (1.0 - hz).prod(dim=0), "min_solvable_fraction": lowest,
            "mean_solvable_fraction": mean, "refills": refills}


def _evaluate_sequential(agent, num_episodes: int, deterministic: bool, render: bool, seed: int,
                         record_actions: bool = False):
    from environment.block_blast_env import BlockBlastEnv

    env = BlockBlastEnv(render_mode="human" if render else None, seed=seed)
    scores, lengths, lines, combos, actions = [], [], [], [], []
    for ep in range(num_episodes):
        obs, info = env.reset(seed=seed + ep)
        done, n, score = False, 0, 0
        actions.append([])
        while not done:
            action, _ = agent.select_action(obs, deterministic=deterministic)
            actions[-1].append(int(action))
            obs, _, terminated, truncated, info = env.step(action)
            done = terminated or truncated
            n += 1
            if render:
                env.render()
            if done:
                score = info.get("score", 0)
        scores.append(score)
        lengths.append(n)
        lines.append(info.get("lines_cleared", 0))
        combos.append(info.get("max_combo", 0))
    env.close()
    res = _summary(scores, lengths, lines, combos)
    if record_actions:
        res["actions"] = actions
    return res


def evaluate_agent(agent, num_episodes: int = 100, deterministic: bool = True, render: bool = False,
                   seed: int = 42, max_moves: int = 100_000, record_actions: bool = False,
                   safe_mask: bool = False, seeds=None, census: bool = False) -> Dict[str, Any]:
    """evaluate.py:23-90 (same keys in the returned dict).  record_actions: also return every episode's
    action sequence under "actions" (for replaying the games elsewhere, e.g. through the oracle).  A game still
    running after max_moves moves is cut off there and reports its score, lines and max combo so far.
    safe_mask: an ``act_device`` agent samples under the legal mask AND the hand-safe mask (the legal mask alone
    where no move is safe); an ``act_env`` agent chooses its own mask (``RandomAgent(safe=True)``).
    seeds: one seed per episode (a list of num_episodes ints) in place of ``seed + e``, e.g. the same piece stream
    for several episodes (``evaluation/tune.py``); not with render.
    census: after every step that leaves an unfinished game with a whole hand -- a refill has just happened -- take
    the refill census of the live boards (one ``bb_refill_census`` launch over all episodes; the games start together
    and never reset, so their refills fall on the same steps).  It describes the deal before it was made: the hand
    that was dealt is not read.  The result gains the CENSUS_KEYS as per-episode lists and their means as
    "mean_<key>" (``census_summary``); not with render.  Without it the result is what it was."""
    agent.eval()
    if seeds is None:
        seeds = [seed + e for e in range(num_episodes)]
    elif render or len(seeds) != num_episodes:
        raise ValueError("evaluate_agent: seeds needs one seed per episode and excludes render")
    if census and render:
        raise ValueError("evaluate_agent: census excludes render")
    if render:
        return _evaluate_sequential(agent, num_episodes, deterministic, render, seed, record_actions)
    from runtime.device_env import DeviceEnvBatch

    dev = agent.device
    n = num_episodes
    env = DeviceEnvBatch(n, [int(sd) for sd in seeds], autoreset=False, device=dev)
    env.reset()
    x = torch.zeros((n, 4, 8, 8), dtype=torch.float32, device=dev)
    mb = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    safe_bits = torch.zeros_like(mb) if safe_mask else None
    act = torch.zeros(n, dtype=torch.int32, device=dev)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    rec = torch.zeros((n, 4), dtype=torch.int64, device=dev)  # score, lines, max_combo, done
    info64 = env.info.view(torch.int64).view(n, 7)
    info32 = env.info.view(torch.int32).view(n, 14)
    log = []
    if census:
        hand = torch.zeros(n, dtype=torch.int32, device=dev)
        count = torch.zeros(n, dtype=torch.int32, device=dev)
        census_rows = []
    act_env = getattr(agent, "act_env", None)
    for step in range(max_moves):
        if act_env is not None:
            act_env(env, act)
        else:
            env.obs(x=x, mask_bits=mb)
            if safe_mask:
                from agents.greedy import apply_safe_mask

                apply_safe_mask(env, mb, safe_bits)
            a, _, _ = agent.act_device(x, mb, deterministic=deterministic)
            act.copy_(a)
        if record_actions:
            log.append(act.clone())
        env.step(act, want_info=True)
        length += alive.long()
        term = env.terminated.bool() & alive
        rec[:, 0] = torch.where(term, info64[:, 0], rec[:, 0])
        rec[:, 1] = torch.where(term, info32[:, 7].long(), rec[:, 1])
        rec[:, 2] = torch.where(term, info32[:, 8].long(), rec[:, 2])
        alive &= ~term
        if census and step % 3 == 2:  # every game is on the third move of a hand, or over
            env.snapshot(hand=hand)
            env.refill_census(count=count)
            whole = ((hand >> 18) & 7) == 0  # nothing of the hand used: it is a new one
            census_rows.append(torch.where(alive & whole, count.long(), torch.full_like(count, -1, dtype=torch.int64)))
        if step % 16 == 15 and not bool(alive.any()):
            break
    if bool(alive.any()):  # games cut off by max_moves: their statistics so far (a finished game latched its own)
        st = env.state()
        for col, key in enumerate(("score", "lines", "max_combo")):
            rec[:, col] = torch.where(alive, torch.from_numpy(st[key].astype(np.int64)).to(dev), rec[:, col])
    out = rec.cpu().numpy()
    lengths = length.cpu().numpy()
    env.close()
    res = _summary(out[:, 0].tolist(), lengths.tolist(), out[:, 1].tolist(), out[:, 2].tolist())
    if record_actions:
        acts = torch.stack(log).cpu().numpy() if log else np.zeros((0, n), np.int32)
        res["actions"] = [acts[:int(lengths[e]), e].tolist() for e in range(n)]
    if census:
        rows = torch.stack(census_rows).cpu() if census_rows else torch.zeros((0, n), dtype=torch.int64)
        for k, v in census_summary(rows).items():
            res[k] = v.tolist()
            res[f"mean_{k}"] = float(v.double().mean())
    return res


def print_census(results: Dict[str, Any]) -> None:
    """The census lines of the summary (``--census``)."""
    print("\nRefill census:")
    print(f"  Mean refills: {results['mean_refills']:.1f}")
    print(f"  Expected lost deals per game: {results['mean_expected_losses']:.3e}")
    print(f"  Mean survival probability: {results['mean_survival']:.6f}")
    print(f"  Solvable fraction: mean {results['mean_mean_solvable_fraction']:.4f}, "
          f"lowest {min(results['min_solvable_fraction']):.4f}")


def print_results(results: Dict[str, Any]) -> None:
    """evaluate.py:93-117."""
    print("\n" + "=" * 60)
    print("EVALUATION RESULTS")
    print("=" * 60)
    print(f"Episodes: {results['num_episodes']}")
    print()
    print("Score Statistics:")
    print(f"  Mean:   {results['mean_score']:.1f} ± {results['std_score']:.1f}")
    print(f"  Median: {results['median_score']:.1f}")
    print(f"  Min:    {results['min_score']:.1f}")
    print(f"  Max:    {results['max_score']:.1f}")
    print()
    print("Game Statistics:")
    print(f"  Mean length: {results['mean_length']:.1f} ± {results['std_length']:.1f}")
    print(f"  Mean lines cleared: {results['mean_lines_cleared']:.1f}")
    print(f"  Mean max combo: {results['mean_max_combo']:.1f}")
    print("=" * 60)
    print("\nScore Percentiles:")
    for p in (10, 25, 50, 75, 90, 95, 99):
        print(f"  {p}th: {np.percentile(results['scores'], p):.1f}")


def main() -> None:
    """evaluate.py:119-184 (same flags)."""
    ap = argparse.ArgumentParser(description="Evaluate Block Blast AI")
    ap.add_argument("--agent", choices=("ppo", "greedy", "plan", "plan2", "playout", "random"), default="ppo",
                    help="ppo: the checkpoint's policy; greedy / plan / plan2 / random: the untrained baselines "
                         "(plan: exhaustive search over the whole hand; plan2: that search with a sampled look past "
                         "the refill, dealt next hands searched below its best first moves; playout: plan2 with "
                         "every deal played on for --hands hands)")
    ap.add_argument("--depth", type=int, choices=(1, 2, 3), default=3, help="--agent plan / plan2: moves searched ahead")
    ap.add_argument("--candidates", type=int, default=8,
                    help="--agent plan2: first moves looked past the refill (untuned default)")
    ap.add_argument("--deals", type=int, default=16,
                    help="--agent plan2 / playout: next hands dealt per candidate (untuned default)")
    ap.add_argument("--hands", type=int, default=2,
                    help="--agent playout: hands dealt, searched and played per playout (untuned default)")
    ap.add_argument("--checkpoint", type=str, default=None, help="required for --agent ppo")
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--output", type=str, default=None)
    ap.add_argument("--max-moves", type=int, default=100_000, help="cut every game off after this many moves")
    ap.add_argument("--weights", type=str, default=None,
                    help="--agent greedy / plan: a JSON file the agent's save wrote")
    ap.add_argument("--device", type=str, default=None, help="baselines only: cpu = the host backend")
    ap.add_argument("--safe-mask", action="store_true",
                    help="--agent ppo / random: choose among hand-safe actions only (the legal moves after which "
                         "the rest of the hand still fits), among the legal ones where none is safe")
    ap.add_argument("--census", action="store_true",
                    help="price every refill: the exact probability that the deal fails on the board as it stands "
                         "(expected lost deals, survival, solvable fractions per game)")
    args = ap.parse_args()
    if args.agent == "ppo":
        if args.checkpoint is None:
            ap.error("--checkpoint is required for --agent ppo")
        if not os.path.exists(args.checkpoint):
            print(f"Checkpoint not found: {args.checkpoint}")
            sys.exit(1)
        from agents.ppo import PPOAgent
        from utils.device import get_device

        agent = PPOAgent(device=get_device())
        agent.load(args.checkpoint)
        print(f"Loaded model from {args.checkpoint}")
    else:
        from agents.greedy import GreedyAgent, HandPlanAgent, PlayoutPlanAgent, RandomAgent, two_hand_agent_class

        if args.agent == "plan":
            agent = HandPlanAgent(device=args.device)
        elif args.agent == "plan2":
            named = None
            if args.weights:  # a file that names a shape weight other than 0 is played by TwoHandShapeAgent
                with open(args.weights) as f:
                    named = json.load(f).get("weights")
            agent = two_hand_agent_class(named)(seed=args.seed, device=args.device)
        elif args.agent == "playout":
            agent = PlayoutPlanAgent(seed=args.seed, device=args.device)
        else:
            agent = (GreedyAgent(device=args.device) if args.agent == "greedy"
                     else RandomAgent(device=args.device, safe=args.safe_mask))
        if args.weights:
            agent.load(args.weights)
        if args.agent in ("plan", "plan2", "playout"):
            agent.depth = args.depth
        if args.agent in ("plan2", "playout"):  # the command line decides, as it does for --depth
            agent.candidates, agent.deals = args.candidates, args.deals
        if args.agent == "playout":
            if not 1 <= args.hands <= 256:
                ap.error("--hands must be 1..256")
            agent.hands = args.hands
        print(f"Baseline agent: {args.agent}" + (" (hand-safe actions)" if getattr(agent, "safe", False) else ""))
    res = evaluate_agent(agent, num_episodes=args.episodes, deterministic=args.deterministic, render=args.render,
                         seed=args.seed, max_moves=args.max_moves, safe_mask=args.safe_mask,
                         **({"census": True} if args.census else {}))
    print_results(res)
    if args.census:
        print_census(res)
    if args.output:
        with open(args.output, "w") as f:
            json.dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}, f, indent=2,
                      default=float)
        print(f"\nResults saved to {args.output}")


if __name__ == "__main__":
    main()
