"""Tuning the eight integer weights of the search agents (``agents/greedy.py``) by playing.

The reference has no search agent and so nothing to tune.  ``GreedyAgent`` / ``HandPlanAgent`` choose their moves by an
integer value of eight weights (bb_greedy_weights); which weights score best is found here by the cross-entropy
method (CEM) over whole games: a population of candidate weight vectors plays the same piece streams, the best
quarter refits a diagonal Gaussian, and so on.  What makes this cheap is ``bb_plan_actions_each``: one search launch
per move serves the whole population, every env with the weights of its candidate (``PopulationPlanAgent``).

``evaluate_population``  final scores int64 [P, G] of P candidates on G shared piece streams, one env batch; with
                         ``census=True`` also what the refill census says of every game (``bb_refill_census``)
``cem``                  the objective-agnostic core (float64 on the host, integer candidates)
``tune``                 CEM with the mean score as fitness, or (``fitness="survival"``) the score discounted by the
                         probability of surviving ``horizon`` moves; writes the agents' weights JSON and a JSONL log
``compare``              score per move of several weight sets on shared held-out games
``compare_two_hand``     the same records with every set played by a ``TwoHandPlanAgent`` (``--compare ... --agent
                         plan2 --candidates K --deals M``; both defaults, 8 and 16, are untuned), or with ``--agent
                         playout --hands H`` by a ``PlayoutPlanAgent`` (H untuned as well)
``playout_scores``       whole games of the plan agent under a counter-based dealer, every candidate and game in one
                         ``bb_playout_values`` launch; ``tune(engine="playout")`` takes a generation's fitness from it

Every default below (population 64, 8 games, 300 moves, 30 generations, elite fraction 0.25, sigma0 300, scale 1000,
sigma floor 10, 32 held-out games, ``dead`` fixed, and for ``fitness="survival"`` the form score * survival **
(horizon / length) and horizon = moves) is a starting point chosen by reasoning: none of them has been tuned.
Playing strength is reported, never asserted.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from agents.greedy import DEFAULT_WEIGHTS, PopulationPlanAgent, PopulationTwoHandAgent
from runtime import kernels as K
from runtime import lib as L

from .evaluate import evaluate_agent

HOLDOUT_SEED_OFFSET = 10 ** 6  # the held-out games of ``tune`` are seeded seed + 10**6 + g


EXTRAS = ("expected_losses", "survival", "min_solvable_fraction", "refills")  # evaluate_population(census=True)


def _play_population(weight_dicts: Sequence[Dict[str, int]], games: int, moves: int, seed: int, depth: int, device,
                     census: bool = False, two_hand: Optional[Dict[str, int]] = None):
    """(scores, lengths, extras), int64 [P, G] each: env c * G + g plays candidate c on the piece stream seeded
    seed + g.  extras: None, or with census the EXTRAS of ``evaluate_agent(census=True)`` as [P, G] tensors.
    ``two_hand`` ({"candidates", "deals"}): the population is played by a ``PopulationTwoHandAgent`` under rows of
    twelve, env e with stream id e % G -- the candidates of a game meet the same dealt hands -- and the deals keyed by
    ``seed``: row c is what ``two_hand_agent_class(w_c)(w_c, depth, candidates, deals, seed)`` scores on the G games."""
    p, g = len(weight_dicts), int(games)
    if two_hand is not None:
        rows = K.eval_rows(list(weight_dicts)).repeat_interleave(g, dim=0)
        agent = PopulationTwoHandAgent(rows, depth=depth, candidates=int(two_hand["candidates"]),
                                       deals=int(two_hand["deals"]), seed=seed,
                                       stream=torch.arange(p * g, dtype=torch.int64) % g, device=device)
    elif any(set(w) & set(L.TERM_FIELDS) for w in weight_dicts):  # a shape weight is named: rows of twelve
        rows = K.eval_rows(list(weight_dicts)).repeat_interleave(g, dim=0)
        agent = PopulationPlanAgent(rows, depth=depth, device=device)
    else:
        rows = K.weight_rows(list(weight_dicts)).repeat_interleave(g, dim=0)
        agent = PopulationPlanAgent(rows, depth=depth, device=device)
    res = evaluate_agent(agent, num_episodes=p * g, seeds=[seed + e % g for e in range(p * g)], max_moves=int(moves),
                         **({"census": True} if census else {}))
    extras = None
    if census:
        extras = {k: torch.tensor(res[k], dtype=torch.int64 if k == "refills" else torch.float64).view(p, g)
                  for k in EXTRAS}
    return (torch.tensor(res["scores"], dtype=torch.int64).view(p, g),
            torch.tensor(res["lengths"], dtype=torch.int64).view(p, g), extras)


def evaluate_population(weight_dicts: Sequence[Dict[str, int]], games: int, moves: int, seed: int, depth: int = 3,
                        device=None, census: bool = False, two_hand: Optional[Dict[str, int]] = None):
    """The final score of every (candidate, game): int64 [P, G] on the CPU.  One ``DeviceEnvBatch`` of P * G envs
    without auto-reset; candidate c, game g is seeded ``seed + g`` -- common random numbers: every candidate sees the
    same G piece streams, so candidates differ by their play alone.  The accounting is ``evaluate_agent``'s: the
    score latched at termination, the score so far for a game cut off after ``moves`` moves.  ``depth`` 1..3 searches
    with ``bb_plan_actions_each``, 0 uses the one-ply greedy kernel.  Row c equals the ``scores`` of
    ``evaluate_agent(HandPlanAgent(weight_dicts[c], depth), num_episodes=G, seed=seed, max_moves=moves)`` when the
    dict names all eight weights (a HandPlanAgent fills missing ones from DEFAULT_WEIGHTS, a row with zeros).
    census=True: returns (scores, extras), extras holding float64 [P, G] tensors "expected_losses", "survival",
    "min_solvable_fraction" and an int64 "refills" (``evaluation.evaluate.census_summary``).  The envs of a population
    run without auto-reset and start together, so every live game refills on the same moves: one
    ``bb_refill_census`` launch per three moves over all P * G boards, finished games masked.  ``two_hand``
    ({"candidates", "deals"}): the two-hand agents instead (``PopulationTwoHandAgent``, one ``bb_plan2_values`` call per
    move); row c then equals the ``scores`` of ``evaluate_agent`` of ``two_hand_agent_class(w)(w, depth, candidates,
    deals, seed)`` on the same seeds."""
    scores, _, extras = _play_population(weight_dicts, games, moves, seed, depth, device, census, two_hand)
    return (scores, extras) if census else scores


def survival_fitness(scores: torch.Tensor, lengths: torch.Tensor, survival: torch.Tensor, horizon: int) -> torch.Tensor:
    """``tune(fitness="survival")``'s objective per candidate, float64 [P]: the mean over games of
    score_g * survival_g ** (horizon / max(length_g, 1)) -- the score discounted by the probability, at the hazard
    rate the game showed over its own length, of getting through ``horizon`` moves without a lost deal."""
    expo = float(horizon) / lengths.clamp(min=1).double()
    return (scores.double() * survival.double() ** expo).mean(dim=1)


def normalise(theta: np.ndarray, free: Sequence[int], scale: float) -> np.ndarray:
    """theta with its free coordinates scaled so that the largest of them is ``scale`` in magnitude (left alone
    when they are all zero).  The arg-max of the agents' value does not change under a positive scaling of all
    weights; fixing the scale keeps a search over integers from drifting towards large or unresolvably small ones.
    Fixed coordinates are not touched."""
    out = np.array(theta, dtype=np.float64)
    free = list(free)
    top = np.max(np.abs(out[..., free]), axis=-1, keepdims=True)
    out[..., free] = out[..., free] * np.where(top > 0, scale / np.where(top > 0, top, 1.0), 1.0)
    return out


def cem(fitness: Callable[[np.ndarray, int], np.ndarray], mean0, sigma0, population: int, elite_frac: float,
        generations: int, rng: np.random.Generator, free: Sequence[int], scale: float = 1000,
        sigma_floor: float = 10) -> List[dict]:
    """The cross-entropy method over integer vectors, maximising ``fitness``; float64 on the host.

    mean0: the start vector [D]; the coordinates in ``free`` are searched, the others stay at mean0's values in every
    candidate.  sigma0: a scalar or [len(free)].  The mean's free part is brought to ``scale`` first (``normalise``).
    Generation k: candidate 0 is the current mean itself, candidates 1..population-1 are mean + sigma * N(0, 1) on
    the free coordinates (one ``rng.standard_normal((population - 1, len(free)))`` draw per generation); every
    candidate is normalised to ``scale`` and rounded to integers (``np.rint``), and ``fitness(candidates int64 [P, D],
    k)`` returns [P] floats.  The elites are the top ceil(population * elite_frac) by fitness, ties to the lower index
    (a stable sort); the new mean and sigma are the mean and the population standard deviation (ddof 0) of the
    elites' integer free coordinates, sigma floored at ``sigma_floor``.  Returns one record per generation:
    candidates, fitness, elite (indices, best first), mean and sigma (full [D] / [len(free)], after the update),
    best_fitness, mean_fitness.  The same rng state gives the same history."""
    free = list(free)
    mean = normalise(np.asarray(mean0, dtype=np.float64), free, scale)
    sigma = np.broadcast_to(np.asarray(sigma0, dtype=np.float64), (len(free),)).copy()
    n_elite = max(1, math.ceil(population * elite_frac))
    history = []
    for k in range(generations):
        cand = np.tile(mean, (population, 1))
        cand[1:, free] = mean[free] + sigma * rng.standard_normal((population - 1, len(free)))
        cand = np.rint(normalise(cand, free, scale)).astype(np.int64)
        fit = np.asarray(fitness(cand, k), dtype=np.float64)
        elite = np.argsort(-fit, kind="stable")[:n_elite]
        mean = mean.copy()
        mean[free] = cand[elite][:, free].astype(np.float64).mean(axis=0)
        sigma = np.maximum(cand[elite][:, free].astype(np.float64).std(axis=0), sigma_floor)
        history.append({"generation": k, "candidates": cand, "fitness": fit, "elite": elite, "mean": mean.copy(),
                        "sigma": sigma.copy(), "best_fitness": float(fit.max()), "mean_fitness": float(fit.mean())})
    return history


def _dict_of(theta, fields: Sequence[str] = L.GREEDY_FIELDS) -> Dict[str, int]:
    return {k: int(v) for k, v in zip(fields, theta)}


def _agent_depth(agent: str, depth: int) -> int:
    if agent not in ("plan", "greedy", "plan2"):
        raise ValueError(f"agent must be 'plan', 'plan2' or 'greedy', not {agent!r}")
    if agent != "greedy" and int(depth) not in (1, 2, 3):
        raise ValueError(f"depth must be 1, 2 or 3, not {depth}")
    return int(depth) if agent != "greedy" else 0  # 0: PopulationPlanAgent's one-ply greedy kernel


def _extras_means(extras: Dict[str, torch.Tensor], c: int) -> Dict[str, float]:
    """Candidate c's EXTRAS as columns: expected_losses summed over its games (to stand beside a count of ended
    games), the others averaged, min_solvable_fraction as the lowest of its games."""
    return {"expected_losses": float(extras["expected_losses"][c].sum()),
            "survival": float(extras["survival"][c].mean()),
            "min_solvable_fraction": float(extras["min_solvable_fraction"][c].min()),
            "refills": float(extras["refills"][c].double().mean())}


def compare(weight_dicts: Sequence[Dict[str, int]], games: int, moves: int, seed: int, depth: int = 3,
            device=None, census: bool = False, two_hand: Optional[Dict[str, int]] = None) -> List[dict]:
    """Several weight sets on the same ``games`` piece streams (seeds seed + g), one population call: per set the mean
    score, the mean score per move (each game's score over its own moves) and its standard error over the games, and
    the number of games that ended before the ``moves`` cut.  census=True adds four columns: expected_losses (the
    hazards of all the set's refills summed over its games -- the number of games the census expects the dealer to
    have lost, beside ended_before_cut), survival (mean), min_solvable_fraction (lowest) and refills (mean).
    ``two_hand``: as ``evaluate_population``."""
    scores, lengths, extras = _play_population(weight_dicts, games, moves, seed, depth, device, census, two_hand)
    return _compare_records(weight_dicts, scores, lengths, extras, games, moves)


def _compare_records(weight_dicts, scores, lengths, extras, games: int, moves: int) -> List[dict]:
    """``compare``'s records from scores / lengths int64 [P, G] and the census extras (or None)."""
    per_move = scores.double() / lengths.clamp(min=1).double()
    return [{"weights": dict(w), "mean_score": float(scores[c].double().mean()),
             "mean_length": float(lengths[c].double().mean()),
             "ended_before_cut": int((lengths[c] < int(moves)).sum()),
             "score_per_move": float(per_move[c].mean()),
             "score_per_move_se": float(per_move[c].std(unbiased=True) / math.sqrt(games)) if games > 1 else 0.0,
             **(_extras_means(extras, c) if extras is not None else {})}
            for c, w in enumerate(weight_dicts)]


def compare_two_hand(weight_dicts: Sequence[Dict[str, int]], games: int, moves: int, seed: int, depth: int = 3,
                     candidates: int = 8, deals: int = 16, device=None, census: bool = False,
                     hands: Optional[int] = None) -> List[dict]:
    """``compare`` with every weight set played by a ``TwoHandPlanAgent(depth, candidates, deals)`` (``--agent
    plan2``): the same games (seeds seed + g) and the same records.  The agent takes one weight set, so the sets are
    played one after another, ``games`` envs each, and every agent's deals are keyed by ``seed``.  A set that names a
    shape weight other than 0 is played by a ``TwoHandShapeAgent``.  ``hands`` (``--agent playout --hands H``): every
    set is played by a ``PlayoutPlanAgent`` of that many hands per dealt playout instead."""
    from agents.greedy import PlayoutPlanAgent, two_hand_agent_class

    rows = []
    for w in weight_dicts:
        if hands is not None:
            agent = PlayoutPlanAgent(w, depth=depth, candidates=candidates, deals=deals, hands=int(hands), seed=seed,
                                     device=device)
        else:
            agent = two_hand_agent_class(w)(w, depth=depth, candidates=candidates, deals=deals, seed=seed,
                                            device=device)
        rows.append(evaluate_agent(agent, num_episodes=int(games), seeds=[seed + g for g in range(int(games))],
                                   max_moves=int(moves), **({"census": True} if census else {})))
    scores = torch.tensor([r["scores"] for r in rows], dtype=torch.int64)
    lengths = torch.tensor([r["lengths"] for r in rows], dtype=torch.int64)
    extras = None
    if census:
        extras = {k: torch.tensor([r[k] for r in rows], dtype=torch.int64 if k == "refills" else torch.float64)
                  for k in EXTRAS}
    return _compare_records(weight_dicts, scores, lengths, extras, games, moves)


def playout_scores(rows: torch.Tensor, games: int, hands: int, seed: int, depth: int = 3, device=None):
    """Whole games of the plan agent under a counter-based dealer, all in one ``bb_playout_values`` launch: from N
    empty boards, board i under rows[i] (int32 [N, 12], ``runtime.kernels.eval_rows``), ``games`` playouts of up to
    ``hands`` hands each, stream id 0 for every board -- candidate i's game g meets the hands candidate j's game g
    meets, as long as both accept them (common random numbers).  Game g of every candidate is dealt hand h as deal g
    under Philox key seed + h.  Returns (score, plies, status), int64 / int32 / int32 [N, games] where the rows were
    moved to (``device``, default the GPU): the score and the plies played when the game stopped, and the last hand's
    status word (``K.PLAY_REFILL`` set: the game outlived all ``hands`` hands).  The dealer is not the env's: a hand is
    the first of 100 Philox draws that can be placed in some order (``refill_values``), never an env's PCG64 stream,
    so these scores rank candidates and are not the scores ``evaluate_population`` reports."""
    from runtime.device_env import resolve_device

    dev = resolve_device(device)
    rows = rows.to(dev).contiguous()
    n = rows.shape[0]
    board = torch.zeros(n, dtype=torch.int64, device=dev)
    stream = torch.zeros(n, dtype=torch.int64, device=dev)
    out = K.playout_values(board, rows, int(games), int(hands), seed, stream=stream, depth=int(depth),
                           want=("score", "plies", "status"))
    return out["score"], out["plies"], out["status"]


def tune(agent: str = "plan", depth: int = 3, population: int = 64, games: int = 8, moves: int = 300,
         generations: int = 30, elite_frac: float = 0.25, seed: int = 1, init: Optional[Dict[str, int]] = None,
         fixed: Sequence[str] = ("dead",), device=None, output: Optional[str] = None, log: Optional[str] = None,
         sigma0: float = 300.0, scale: float = 1000, sigma_floor: float = 10, holdout_games: int = 32,
         fitness: str = "score", horizon: Optional[int] = None, terms: Sequence[str] = (), candidates: int = 8,
         deals: int = 16, engine: str = "env") -> dict:
    """CEM over the weights of ``HandPlanAgent(depth)`` (agent "plan"), ``GreedyAgent`` (agent "greedy") or the two-hand
    agent (agent "plan2": ``TwoHandPlanAgent`` / ``TwoHandShapeAgent`` with ``candidates`` and ``deals``, the population
    played by ``PopulationTwoHandAgent``, env e on stream id e % games, every generation's deals keyed by its game seed,
    the held-out comparison played the same way; ``output`` then writes {"agent": "plan2", "depth", "candidates",
    "deals", "seed", "weights"}, which ``TwoHandPlanAgent.load`` reads, and the final record names both numbers).

    Fitness is a candidate's mean final score over ``games`` games of at most ``moves`` moves
    (``evaluate_population``).  Generation k plays the seeds ``seed + k * games + g``: fresh for each generation,
    shared by all its candidates.  ``init`` (default DEFAULT_WEIGHTS) is the start mean; the weights named in
    ``fixed`` keep init's values.  After the last generation one population call with P = 2 plays ``init`` against
    the final weights (the last mean, normalised and rounded) on ``holdout_games`` held-out games seeded from
    ``seed + 10**6``.  ``output``: the final weights in the agents' JSON format ({"agent", "depth", "weights"};
    ``HandPlanAgent.load`` / ``evaluate.py --weights`` read it).  ``log``: a JSONL file, one "generation" record per
    generation (seeds, best and mean fitness, the best candidate, the mean vector and sigma after the update,
    candidate 0 = the mean as it was played and its fitness) and one "final" record (the weights, the held-out comparison,
    the settings, the build id).  Deterministic for a given ``seed``: the sampling is numpy's ``default_rng(seed)``,
    the games are seeded, the search is exact.  Every default is untuned (see the module docstring).  Returns the
    final record.

    ``fitness="survival"`` maximises ``survival_fitness`` instead: the mean over games of score_g * survival_g **
    (horizon / max(length_g, 1)), survival_g from the refill census of the game's boards
    (``evaluate_population(census=True)``); ``horizon`` defaults to ``moves``.  Its generation records gain
    "mean_played_extras" and "best_extras" (the per-candidate means of the extras), the held-out comparison the
    census columns, and the final record "fitness" and "horizon".  With ``fitness="score"`` the records are what they
    were.  The form of the objective and the horizon are untuned.

    ``terms``: names of ``L.TERM_FIELDS`` (perimeter, room3, room5, fits) to add to the searched vector (agent "plan"
    only: the search with them is ``bb_plan_actions_ext``).  They start at init's value, 0 by default, and share
    sigma0 and the normalisation with the eight; the dicts of the records then carry them and the settings name
    them.  With no terms every record, candidate and random draw is what it was.

    ``engine="playout"`` (agent "plan", fitness "score"): a generation's fitness is the row mean of
    ``playout_scores`` -- every candidate's ``games`` games of hands = ceil(moves / 3) hands in one launch, under the
    counter-based dealer and keyed by ``TwoHandPlanAgent.deal_seed(seed, k)`` for generation k -- where the default
    engine "env" plays the envs move by move.  The held-out comparison is played by the envs either way, and the final
    record's settings name the engine and the hands.  What the engine does to the weights found is unmeasured."""
    if engine not in ("env", "playout"):
        raise ValueError(f"engine must be 'env' or 'playout', not {engine!r}")
    playout_hands = 0
    if engine == "playout":
        if agent != "plan" or fitness != "score":
            raise ValueError("engine 'playout' plays the plan agent for its score: agent 'plan', fitness 'score'")
        playout_hands = -(-int(moves) // 3)
        if not 1 <= playout_hands <= L.BB_PLAYOUT_MAX_HANDS:
            raise ValueError(f"engine 'playout': hands must be 1..{L.BB_PLAYOUT_MAX_HANDS}, not ceil({moves} / 3) = "
                             f"{playout_hands}")
    if fitness not in ("score", "survival"):
        raise ValueError(f"fitness must be 'score' or 'survival', not {fitness!r}")
    terms = tuple(terms)
    if set(terms) - set(L.TERM_FIELDS) or len(set(terms)) != len(terms):
        raise ValueError(f"terms must be distinct names of {L.TERM_FIELDS}, not {list(terms)}")
    if terms and agent == "greedy":
        raise ValueError("terms need agent 'plan' or 'plan2': the one-ply greedy kernel has no extended form")
    two_hand = None
    if agent == "plan2":
        if not 1 <= int(candidates) <= 192 or not 1 <= int(deals) <= L.BB_REFILL_MAX_DEALS:
            raise ValueError(f"candidates must be 1..192 and deals 1..{L.BB_REFILL_MAX_DEALS}, not {candidates}, {deals}")
        two_hand = {"candidates": int(candidates), "deals": int(deals)}
    th = {"two_hand": two_hand} if two_hand else {}
    fields = L.GREEDY_FIELDS + tuple(k for k in L.TERM_FIELDS if k in terms)
    priced = fitness == "survival"
    horizon = int(moves) if horizon is None else int(horizon)
    extras_log: Dict[int, dict] = {}
    eval_depth = _agent_depth(agent, depth)
    init = dict(DEFAULT_WEIGHTS) if init is None else {**{k: 0 for k in L.GREEDY_FIELDS}, **init}
    if terms:
        init = {**{k: 0 for k in fields}, **init}
        if set(init) - set(fields):
            raise ValueError(f"unknown init weights {sorted(set(init) - set(fields))}; the fields are {fields}")
    else:
        L.greedy_weights(init)  # rejects unknown names
    unknown = set(fixed) - set(fields)
    if unknown:
        raise ValueError(f"unknown fixed weights {sorted(unknown)}; the fields are {fields}")
    free = [i for i, k in enumerate(fields) if k not in fixed]
    mean0 = np.array([init[k] for k in fields], dtype=np.float64)
    t0 = time.perf_counter()

    def objective(cand: np.ndarray, k: int) -> np.ndarray:
        sets = [_dict_of(c, fields) for c in cand]
        if playout_hands:
            from agents.greedy import TwoHandPlanAgent

            score, _, _ = playout_scores(K.eval_rows(sets), games, playout_hands,
                                         TwoHandPlanAgent.deal_seed(seed, k), eval_depth, device)
            return score.double().mean(dim=1).cpu().numpy()
        if not priced:
            scores = evaluate_population(sets, games, moves, seed + k * games, eval_depth, device, **th)
            return scores.double().mean(dim=1).numpy()
        scores, lengths, extras = _play_population(sets, games, moves, seed + k * games, eval_depth, device, True, **th)
        extras_log[k] = {key: extras[key].double().mean(dim=1).tolist() for key in EXTRAS}
        return survival_fitness(scores, lengths, extras["survival"], horizon).numpy()

    history = cem(objective, mean0, sigma0, population, elite_frac, generations, np.random.default_rng(seed), free,
                  scale=scale, sigma_floor=sigma_floor)
    final_theta = np.rint(normalise(history[-1]["mean"] if history else mean0, free, scale)).astype(np.int64)
    weights = _dict_of(final_theta, fields)
    held = compare([init, weights], holdout_games, moves, seed + HOLDOUT_SEED_OFFSET, eval_depth, device,
                   **({"census": True} if priced else {}), **th)
    host = device is not None and torch.device(device).type == "cpu"
    final = {"record": "final", "agent": agent, "depth": int(depth) if agent != "greedy" else None, "weights": weights,
             "init": init, "fixed": list(fixed),
             "holdout": {"seed0": seed + HOLDOUT_SEED_OFFSET, "games": holdout_games, "moves": moves,
                         "init": held[0], "tuned": held[1]},
             "settings": {"population": population, "games": games, "moves": moves, "generations": generations,
                          "elite_frac": elite_frac, "seed": seed, "sigma0": sigma0, "scale": scale,
                          "sigma_floor": sigma_floor},
             "build_id": L.build_id(host=host), "backend": "host" if host else "hip",
             "wall_s": round(time.perf_counter() - t0, 3)}
    if priced:
        final["fitness"], final["horizon"] = fitness, horizon
    if terms:
        final["settings"]["terms"] = list(fields[len(L.GREEDY_FIELDS):])
    if two_hand:
        final["settings"].update(two_hand)
    if playout_hands:
        final["settings"].update(engine=engine, hands=playout_hands)
    if output:
        doc = {"agent": agent, "weights": weights}
        if agent == "plan":
            doc = {"agent": agent, "depth": int(depth), "weights": weights}
        if agent == "plan2":
            doc = {"agent": agent, "depth": int(depth), "candidates": int(candidates), "deals": int(deals),
                   "seed": int(seed), "weights": weights}
        with open(output, "w") as f:
            json.dump(doc, f, indent=2)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            for h in history:
                best = int(h["elite"][0])
                more = {}
                if priced:
                    ex = extras_log[h["generation"]]
                    more = {"mean_played_extras": {key: ex[key][0] for key in EXTRAS},
                            "best_extras": {key: ex[key][best] for key in EXTRAS}}
                f.write(json.dumps({
                    "record": "generation", "generation": h["generation"],
                    "seeds": [seed + h["generation"] * games + g for g in range(games)],
                    "best_fitness": h["best_fitness"], "mean_fitness": h["mean_fitness"],
                    "mean_played": _dict_of(h["candidates"][0], fields),
                    "mean_played_fitness": float(h["fitness"][0]),
                    "best": _dict_of(h["candidates"][best], fields),
                    "mean": [float(x) for x in h["mean"]], "sigma": [float(x) for x in h["sigma"]], **more}) + "\n")
            f.write(json.dumps(final) + "\n")
    return final


def main() -> None:
    ap = argparse.ArgumentParser(description="Tune the search agents' weights by the cross-entropy method")
    ap.add_argument("--agent", choices=("plan", "greedy", "plan2", "playout"), default="plan",
                    help="plan2: the two-hand agent, a sampled look past the refill; playout (--compare only): the "
                         "same with --hands dealt hands per playout")
    ap.add_argument("--hands", type=int, default=2, help="--compare --agent playout: hands per dealt playout (untuned)")
    ap.add_argument("--engine", choices=("env", "playout"), default="env",
                    help="playout: a generation's fitness from one bb_playout_values launch (agent plan, hands = "
                         "ceil(moves / 3) <= 256) instead of the envs played move by move")
    ap.add_argument("--candidates", type=int, default=8, help="--agent plan2: first moves looked past the refill (untuned)")
    ap.add_argument("--deals", type=int, default=16, help="--agent plan2: next hands dealt per candidate (untuned)")
    ap.add_argument("--depth", type=int, choices=(1, 2, 3), default=3, help="--agent plan: moves searched ahead")
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--games", type=int, default=8, help="games per candidate and generation (shared piece streams)")
    ap.add_argument("--moves", type=int, default=300, help="cut every game off after this many moves")
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--elite-frac", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--holdout-games", type=int, default=32)
    ap.add_argument("--device", type=str, default=None, help="cpu = the host backend")
    ap.add_argument("--output", type=str, default=None, help="the tuned weights, in the agents' JSON format")
    ap.add_argument("--log", type=str, default=None, help="JSONL: one record per generation and a final one")
    ap.add_argument("--compare", type=str, default=None, nargs="+",
                    help="no tuning: play these weights JSON files against DEFAULT_WEIGHTS on --games games seeded "
                         "from --seed")
    ap.add_argument("--census", action="store_true",
                    help="--compare: add the refill census columns (expected_losses, survival, "
                         "min_solvable_fraction, refills)")
    ap.add_argument("--fitness", choices=("score", "survival"), default="score",
                    help="survival: the score discounted by the census' probability of surviving --horizon moves")
    ap.add_argument("--horizon", type=int, default=None, help="--fitness survival: moves to survive (default --moves)")
    ap.add_argument("--terms", type=str, default=None,
                    help="--agent plan / plan2: shape terms to tune beside the eight, comma-separated names of "
                         "perimeter,room3,room5,fits (they start at 0)")
    args = ap.parse_args()
    if args.compare:
        others = []
        for path in args.compare:
            with open(path) as f:
                others.append(json.load(f)["weights"])
        if args.agent in ("plan2", "playout"):
            res = compare_two_hand([dict(DEFAULT_WEIGHTS), *others], args.games, args.moves, args.seed, args.depth,
                                   args.candidates, args.deals, args.device, **({"census": True} if args.census else {}),
                                   **({"hands": args.hands} if args.agent == "playout" else {}))
        else:
            res = compare([dict(DEFAULT_WEIGHTS), *others], args.games, args.moves, args.seed,
                          _agent_depth(args.agent, args.depth), args.device,
                          **({"census": True} if args.census else {}))
        rec = {"record": "compare", "seed0": args.seed, "games": args.games, "moves": args.moves,
               "agent": args.agent, "depth": args.depth, "init": res[0], "other": res[1]}
        if args.agent in ("plan2", "playout"):
            rec.update(candidates=args.candidates, deals=args.deals)
        if args.agent == "playout":
            rec.update(hands=args.hands)
        if len(res) > 2:
            rec["more"] = [{"file": os.path.basename(p), **r} for p, r in zip(args.compare[1:], res[2:])]
        print(json.dumps(rec))
        return
    if args.agent == "playout":
        ap.error("--agent playout is offered with --compare; to tune through playouts use --agent plan --engine playout")
    final = tune(agent=args.agent, depth=args.depth, population=args.population, games=args.games, moves=args.moves,
                 generations=args.generations, elite_frac=args.elite_frac, seed=args.seed,
                 device=args.device, output=args.output, log=args.log, holdout_games=args.holdout_games,
                 **({"fitness": args.fitness, "horizon": args.horizon} if args.fitness != "score" else {}),
                 **({"terms": [t for t in args.terms.split(",") if t]} if args.terms else {}),
                 **({"candidates": args.candidates, "deals": args.deals} if args.agent == "plan2" else {}),
                 **({"engine": args.engine} if args.engine != "env" else {}))
    print(json.dumps(final))


if __name__ == "__main__":
    main()
