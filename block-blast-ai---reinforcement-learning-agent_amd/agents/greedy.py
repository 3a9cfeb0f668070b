"""Baseline agents that need no training: a one-ply greedy heuristic, a full-hand plan search and random legal play.

The reference has no baseline players; these give a checkpoint's evaluation something to be compared with
(``evaluate.py --agent greedy`` / ``--agent random`` on the same seeds).  Both choose their actions on the
device the envs live on: ``GreedyAgent`` through the fused ``bb_greedy_actions`` kernel (the arg-max of an
integer value over the afterstates of the 192 actions, csrc/bb_lookahead.hip), ``RandomAgent`` through the
Philox random-legal policy ``bb_random_actions``.  ``HandPlanAgent`` searches every way to play out the hand
(``bb_plan_actions``, the fused search kernel of the same file; ``evaluate.py --agent plan``).
``TwoHandPlanAgent`` looks past the refill that search stops at: below its best first moves it deals next hands by the
dealer's law and searches them (``bb_play_plan_pos``, ``bb_refill_values``; ``evaluate.py --agent plan2``); ``TwoHandShapeAgent`` is that agent under
the twelve weights (``bb_plan_values_ext``, ``bb_refill_values_ext``).
``PopulationPlanAgent`` is that search with weights of its own for every env (``bb_plan_actions_each``), which
``evaluation/tune.py`` tunes the weights with.  ``HandPlanAgent`` and ``PopulationPlanAgent`` also take the four shape
weights of ``L.TERM_FIELDS`` (perimeter, room3, room5, fits) and then search with ``bb_plan_actions_ext``.
``device="cpu"`` runs them on the host backend.
"""
from __future__ import annotations

import json
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from runtime import lib as L

from .base import BaseAgent

# Chosen by reasoning, not tuned: a cleared line is worth far more than anything else a single move does, new
# holes are the main lasting damage, a fuller board is worse, more placements left for the remaining pieces is
# better, and a move after which the remaining pieces cannot be placed ends the game.
DEFAULT_WEIGHTS = {"lines": 100, "score": 0, "holes": -30, "filled": -2, "centre": 0, "mobility": 1,
                   "dead": -100000, "refill": 0}


def _position_of(observation: Dict[str, Any]):
    """(board bits, packed hand word) of a Gym observation: the board plane and the unused pieces' shapes
    (a used slot's plane is all zeros)."""
    from game.pieces import PIECE_MASKS

    board = np.asarray(observation["board"]).reshape(64) != 0
    bits = int(sum(1 << i for i in np.nonzero(board)[0]))
    hand = 0
    for s, plane in enumerate(np.asarray(observation["pieces"])):
        match = np.nonzero((PIECE_MASKS == plane).all(axis=(1, 2)))[0]
        if match.size:
            hand |= int(match[0]) << (6 * s)
        else:
            hand |= 1 << (18 + s)
    return bits, hand


def apply_safe_mask(env_batch, mask_bits: torch.Tensor, safe_bits: torch.Tensor) -> torch.Tensor:
    """AND the hand-safe mask of a ``DeviceEnvBatch`` (``safe_mask``, written to safe_bits) into its legal mask
    words mask_bits (int64 [N, 3] each), in place; an env without a safe action keeps its legal mask.  No sync."""
    env_batch.safe_mask(safe_bits)
    has_safe = (safe_bits != 0).any(dim=1, keepdim=True)
    mask_bits.copy_(torch.where(has_safe, mask_bits & safe_bits, mask_bits))
    return mask_bits


class GreedyAgent(BaseAgent):
    """Plays the legal action with the largest one-ply greedy value (ties: the lowest action)."""

    def __init__(self, weights: Optional[Dict[str, int]] = None, device=None):
        from runtime.device_env import resolve_device

        super().__init__(resolve_device(device))
        self.weights = dict(DEFAULT_WEIGHTS)
        if weights:
            self._check_weights(weights)  # rejects unknown names
            self.weights.update({k: int(v) for k, v in weights.items()})

    def _check_weights(self, weights: Dict[str, int]) -> None:
        """Rejects names this agent's kernels have no term for.  The shape terms of ``L.TERM_FIELDS`` exist in the
        full-hand search and its per-action and dealt-hand forms (``bb_plan_actions_ext``, ``bb_plan_values_ext``,
        ``bb_refill_values_ext``), which ``HandPlanAgent`` and ``TwoHandShapeAgent`` play through; the one-ply
        ``bb_greedy_actions`` has no extended form."""
        shape = sorted(set(weights) & set(L.TERM_FIELDS))
        if shape:
            raise ValueError(f"{type(self).__name__} has no extended kernel yet: the shape weights {shape} are "
                             f"searched by HandPlanAgent and PopulationPlanAgent only")
        L.greedy_weights(weights)

    def act_env(self, env_batch, out: torch.Tensor) -> torch.Tensor:
        """The action of every env of a ``DeviceEnvBatch`` into out (int32 [N]), in one fused launch."""
        return env_batch.greedy_actions(out, self.weights)

    def select_action(self, observation: Dict[str, Any], deterministic: bool = True) -> Tuple[int, Dict[str, Any]]:
        """From a Gym observation.  The observation does not carry the combo count, so the ``score`` weight (0
        by default) sees every move as the first of a streak here; ``act_env`` reads the real count."""
        from runtime import kernels as K

        bits, hand = _position_of(observation)
        board = torch.tensor([bits - (1 << 64) if bits >= 1 << 63 else bits], dtype=torch.int64, device=self.device)
        hand_t = torch.tensor([hand], dtype=torch.int32, device=self.device)
        action, value = K.greedy_actions(board, hand_t, self.weights)
        return int(action.cpu().item()), {"value": int(value.cpu().item())}

    def update(self, *args, **kwargs) -> Dict[str, float]:
        return {}

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"agent": "greedy", "weights": self.weights}, f, indent=2)

    def load(self, path: str) -> None:
        with open(path) as f:
            data = json.load(f)
        self._check_weights(data["weights"])
        self.weights = dict(DEFAULT_WEIGHTS)
        self.weights.update({k: int(v) for k, v in data["weights"].items()})


class HandPlanAgent(GreedyAgent):
    """Plays the first move of the best way to play out the whole hand: the exhaustive search of
    ``bb_plan_actions`` over every order and placement of the unused pieces, up to ``depth`` (1..3) moves, under
    the same integer weights (move terms summed along the sequence, state terms of its last afterstate; ties:
    the lexicographically lowest sequence).  ``depth=1`` is ``GreedyAgent``.  One fused launch per move.

    The weights may also name the shape terms of ``L.TERM_FIELDS`` (perimeter, room3, room5, fits of the last
    afterstate's board).  When one of them is not 0 the agent searches with ``bb_plan_actions_ext``; otherwise it
    plays through ``bb_plan_actions`` as it always did."""

    def __init__(self, weights: Optional[Dict[str, int]] = None, depth: int = 3, device=None):
        super().__init__(weights, device)
        if int(depth) not in (1, 2, 3):
            raise ValueError(f"depth must be 1, 2 or 3, not {depth}")
        self.depth = int(depth)
        self._rows = None  # the [1, 12] row of plan_actions_ext, made on first use where the positions are

    def _check_weights(self, weights: Dict[str, int]) -> None:
        L.eval_weights(weights)

    def _ext_rows(self, dev) -> Optional[torch.Tensor]:
        """The agent's weights as one shared row of ``plan_actions_ext`` on dev; None when no shape weight is set."""
        if not any(int(self.weights.get(k, 0)) != 0 for k in L.TERM_FIELDS):
            return None
        from runtime import kernels as K

        want = [int(self.weights.get(k, 0)) for k in L.EVAL_FIELDS]
        if self._rows is None or self._rows[0] != want or self._rows[1].device != dev:
            self._rows = (want, K.eval_rows(self.weights, device=dev))
        return self._rows[1]

    def _base_weights(self) -> Dict[str, int]:
        return {k: v for k, v in self.weights.items() if k in L.GREEDY_FIELDS}

    def act_env(self, env_batch, out: torch.Tensor) -> torch.Tensor:
        rows = self._ext_rows(env_batch.device)
        if rows is not None:
            return env_batch.plan_actions_ext(out, rows, self.depth)
        return env_batch.plan_actions(out, self._base_weights(), self.depth)

    def select_action(self, observation: Dict[str, Any], deterministic: bool = True) -> Tuple[int, Dict[str, Any]]:
        """From a Gym observation (no combo count in it: see ``GreedyAgent.select_action``)."""
        from runtime import kernels as K

        bits, hand = _position_of(observation)
        board = torch.tensor([bits - (1 << 64) if bits >= 1 << 63 else bits], dtype=torch.int64, device=self.device)
        hand_t = torch.tensor([hand], dtype=torch.int32, device=self.device)
        rows = self._ext_rows(self.device)
        if rows is not None:
            res = K.plan_actions_ext(board, hand_t, rows, self.depth, want_plan=True)
        else:
            res = K.plan_actions(board, hand_t, self._base_weights(), self.depth, want_plan=True)
        return int(res["action"].cpu().item()), {"value": int(res["value"].cpu().item()),
                                                 "plan": res["plan"].cpu().view(3).tolist()}

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"agent": "plan", "depth": self.depth, "weights": self.weights}, f, indent=2)

    def load(self, path: str) -> None:
        super().load(path)
        with open(path) as f:
            depth = int(json.load(f).get("depth", self.depth))
        if depth not in (1, 2, 3):
            raise ValueError(f"depth must be 1, 2 or 3, not {depth}")
        self.depth = depth


class TwoHandPlanAgent(HandPlanAgent):
    """``HandPlanAgent`` with a sampled look past the refill: a one-chance-node expectimax over the next hand.  Per
    decision, all in integers:

    1. ``plan_values`` at ``depth`` gives q[192] and the rest of the best sequence below every first move;
    2. the candidates are the ``candidates`` legal actions with the largest q (stable descending sort: ties to the
       lower action; fewer legal actions, fewer candidates; none: action 0);
    3. ``play_plan`` on (a, rest[a]) gives each candidate's leaf board, combo, lines, score and status;
    4. a leaf that is a refill is dealt ``deals`` next hands by ``refill_values`` -- stream id = the root position's
       index in the batch, the same for all its candidates, so they meet the same draws (common random numbers); seed
       = ``deal_seed(seed, move counter)`` -- and Q2[a] = deals * (w.lines * lines + w.score * score) + sum of the
       dealt hands' values;
    5. a leaf that is not a refill (the sequence ended dead, or ``depth`` cut it short) keeps Q2[a] = deals * q[a];
    6. the action is the arg-max of Q2, ties to the lower action.

    With ``candidates=1`` it plays what ``HandPlanAgent`` plays.  The defaults (8 candidates, 16 deals) are untuned."""

    def __init__(self, weights: Optional[Dict[str, int]] = None, depth: int = 3, candidates: int = 8, deals: int = 16,
                 seed: int = 0, device=None):
        super().__init__(weights, depth, device)
        if not 1 <= int(candidates) <= 192:
            raise ValueError(f"candidates must be 1..192, not {candidates}")
        if not 1 <= int(deals) <= L.BB_REFILL_MAX_DEALS:
            raise ValueError(f"deals must be 1..{L.BB_REFILL_MAX_DEALS}, not {deals}")
        self.candidates, self.deals, self.seed = int(candidates), int(deals), int(seed)
        self.moves = 0  # decisions made so far: mixed into the deals' seed

    def _check_weights(self, weights: Dict[str, int]) -> None:
        GreedyAgent._check_weights(self, weights)  # plan_values / refill_values have no extended form

    @staticmethod
    def deal_seed(seed: int, move: int) -> int:
        """The Philox key of the deals of decision ``move`` (0-based): seed + (move + 1) * 0x9E3779B97F4A7C15 mod 2^64."""
        return (int(seed) + (int(move) + 1) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)

    # the three kernel calls of a decision, which TwoHandShapeAgent makes under twelve weights
    def _plan_values_env(self, env_batch, out: dict) -> dict:
        return env_batch.plan_values(self.weights, self.depth, out=out)

    def _plan_values_pos(self, board, hand) -> dict:
        from runtime import kernels as K

        return K.plan_values(board, hand, self.weights, self.depth, want=("q", "rest"))

    def _refill_values(self, board, deals: int, seed: int, combo, stream) -> torch.Tensor:
        from runtime import kernels as K

        return K.refill_values(board, self.weights, deals, seed, combo=combo, stream=stream, depth=self.depth)["value"]

    def _decide(self, board, hand, combo, q, rest) -> torch.Tensor:
        """Steps 2-6 for n positions: board i64 / hand i32 / combo i32 [n], q i64 / rest i32 [n, 192] -> int64 [n]."""
        from runtime import kernels as K

        n, k, m = board.numel(), self.candidates, self.deals
        lowest = torch.iinfo(torch.int64).min
        cand = torch.sort(q, dim=1, descending=True, stable=True).indices[:, :k]  # [n, k]
        qc = q.gather(1, cand)
        valid = qc != lowest
        a2, a3 = K.unpack_rest(rest.gather(1, cand))
        plan = torch.stack([cand.to(torch.int32), a2.to(torch.int32), a3.to(torch.int32)], dim=2)
        plan = torch.where(valid.unsqueeze(2), plan, torch.full_like(plan, -1)).view(n * k, 3).contiguous()
        leaf = K.play_plan(board.repeat_interleave(k), hand.repeat_interleave(k), plan, combo.repeat_interleave(k),
                           want=("board", "combo", "lines", "score", "status"))
        refill = ((leaf["status"] & K.PLAY_REFILL) != 0) & valid.view(-1)
        q2 = torch.where(valid, m * qc, torch.full_like(qc, lowest)).view(-1)
        idx = torch.nonzero(refill).view(-1)
        if idx.numel():
            root = torch.arange(n, dtype=torch.int64, device=board.device).repeat_interleave(k)
            v = self._refill_values(leaf["board"][idx].contiguous(), m, self.deal_seed(self.seed, self.moves),
                                    leaf["combo"][idx].contiguous(), root[idx].contiguous())
            moved = self.weights["lines"] * leaf["lines"][idx].long() + self.weights["score"] * leaf["score"][idx]
            q2[idx] = m * moved + v.sum(dim=1)
        q2 = q2.view(n, k)
        best = q2.max(dim=1, keepdim=True).values
        action = torch.where(q2 == best, cand, torch.full_like(cand, 192)).min(dim=1).values
        self.moves += 1
        return torch.where(valid.any(dim=1), action, torch.zeros_like(action))

    def act_env(self, env_batch, out: torch.Tensor) -> torch.Tensor:
        """The action of every env of a ``DeviceEnvBatch`` into out (int32 [N]); one decision of the move counter."""
        n, dev = env_batch.num_envs, env_batch.device
        pv = self._plan_values_env(env_batch, {"q": torch.empty((n, 192), dtype=torch.int64, device=dev),
                                               "rest": torch.empty((n, 192), dtype=torch.int32, device=dev)})
        board = torch.empty(n, dtype=torch.int64, device=dev)
        hand = torch.empty(n, dtype=torch.int32, device=dev)
        combo = torch.empty(n, dtype=torch.int32, device=dev)
        env_batch.snapshot(board=board, hand=hand)
        env_batch.snapshot_combo(combo)
        out.copy_(self._decide(board, hand, combo, pv["q"], pv["rest"]))
        return out

    def select_action(self, observation: Dict[str, Any], deterministic: bool = True) -> Tuple[int, Dict[str, Any]]:
        """From a Gym observation (no combo count in it: see ``GreedyAgent.select_action``)."""
        bits, hand = _position_of(observation)
        board = torch.tensor([bits - (1 << 64) if bits >= 1 << 63 else bits], dtype=torch.int64, device=self.device)
        hand_t = torch.tensor([hand], dtype=torch.int32, device=self.device)
        pv = self._plan_values_pos(board, hand_t)
        action = self._decide(board, hand_t, torch.zeros(1, dtype=torch.int32, device=self.device), pv["q"], pv["rest"])
        return int(action.cpu().item()), {}

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"agent": "plan2", "depth": self.depth, "candidates": self.candidates, "deals": self.deals,
                       "seed": self.seed, "weights": self.weights}, f, indent=2)

    def load(self, path: str) -> None:
        super().load(path)
        with open(path) as f:
            data = json.load(f)
        self.candidates = int(data.get("candidates", self.candidates))
        self.deals = int(data.get("deals", self.deals))
        self.seed = int(data.get("seed", self.seed))


class TwoHandShapeAgent(TwoHandPlanAgent):
    """``TwoHandPlanAgent`` under the twelve weights: its weights (and ``load``'s JSON) may name the shape terms of
    ``L.TERM_FIELDS``.  When one of them is not 0, steps 1 and 4 run ``plan_values_ext`` and ``refill_values_ext``
    under one shared row, made once per device as ``HandPlanAgent`` makes its own, so q and the dealt hands' values
    carry the shape terms of their leaf boards; the move terms of step 4 stay ``weights["lines"]`` and
    ``weights["score"]``.  With the four shape weights 0 it calls exactly what ``TwoHandPlanAgent`` calls."""

    def _check_weights(self, weights: Dict[str, int]) -> None:
        L.eval_weights(weights)

    def _plan_values_env(self, env_batch, out: dict) -> dict:
        rows = self._ext_rows(env_batch.device)
        if rows is not None:
            return env_batch.plan_values_ext(rows, self.depth, out=out)
        return env_batch.plan_values(self._base_weights(), self.depth, out=out)

    def _plan_values_pos(self, board, hand) -> dict:
        from runtime import kernels as K

        rows = self._ext_rows(board.device)
        if rows is not None:
            return K.plan_values_ext(board, hand, rows, self.depth, want=("q", "rest"))
        return K.plan_values(board, hand, self._base_weights(), self.depth, want=("q", "rest"))

    def _refill_values(self, board, deals: int, seed: int, combo, stream) -> torch.Tensor:
        from runtime import kernels as K

        rows = self._ext_rows(board.device)
        if rows is not None:
            return K.refill_values_ext(board, rows, deals, seed, combo=combo, stream=stream, depth=self.depth)["value"]
        return K.refill_values(board, self._base_weights(), deals, seed, combo=combo, stream=stream,
                               depth=self.depth)["value"]


class PlayoutPlanAgent(TwoHandShapeAgent):
    """``TwoHandShapeAgent`` with more than one chance node behind a refill leaf: step 4 values a candidate's leaf by
    ``deals`` dealt playouts of ``hands`` hands each (``playout_values``: deal, search, play the plan found, deal again
    under key seed + h) where the parent searches one dealt hand.  A playout's value is the move terms of the hands
    it played out plus the search value of its last hand, so a board that takes one more hand well and then chokes
    no longer looks like one that keeps taking hands.  Steps 1-3, 5 and 6 and Q2 = deals * moved + the sum of the
    values are the parent's; the playouts always run under the twelve-weight row, which with the shape weights 0
    gives the eight-weight answers.  With ``hands=1`` it plays what ``TwoHandShapeAgent`` plays.  The default
    ``hands=2`` is untuned."""

    def __init__(self, weights: Optional[Dict[str, int]] = None, depth: int = 3, candidates: int = 8, deals: int = 16,
                 hands: int = 2, seed: int = 0, device=None):
        super().__init__(weights, depth, candidates, deals, seed, device)
        if not 1 <= int(hands) <= L.BB_PLAYOUT_MAX_HANDS:
            raise ValueError(f"hands must be 1..{L.BB_PLAYOUT_MAX_HANDS}, not {hands}")
        self.hands = int(hands)
        self._rows12 = None  # the [1, 12] row of playout_values, made on first use where the boards are

    def _refill_values(self, board, deals: int, seed: int, combo, stream) -> torch.Tensor:
        from runtime import kernels as K

        want = [int(self.weights.get(k, 0)) for k in L.EVAL_FIELDS]
        if self._rows12 is None or self._rows12[0] != want or self._rows12[1].device != board.device:
            self._rows12 = (want, K.eval_rows(self.weights, device=board.device))
        return K.playout_values(board, self._rows12[1], deals, self.hands, seed, combo=combo, stream=stream,
                                depth=self.depth)["value"]

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"agent": "playout", "depth": self.depth, "candidates": self.candidates, "deals": self.deals,
                       "hands": self.hands, "seed": self.seed, "weights": self.weights}, f, indent=2)

    def load(self, path: str) -> None:
        super().load(path)
        with open(path) as f:
            hands = int(json.load(f).get("hands", self.hands))
        if not 1 <= hands <= L.BB_PLAYOUT_MAX_HANDS:
            raise ValueError(f"hands must be 1..{L.BB_PLAYOUT_MAX_HANDS}, not {hands}")
        self.hands = hands


def two_hand_agent_class(weights: Optional[Dict[str, int]]):
    """The two-hand agent for a weight set: ``TwoHandShapeAgent`` when it names a shape weight that is not 0,
    ``TwoHandPlanAgent`` otherwise (``evaluate.py --agent plan2``, ``tune.py --compare ... --agent plan2``)."""
    shaped = any(int((weights or {}).get(k, 0)) != 0 for k in L.TERM_FIELDS)
    return TwoHandShapeAgent if shaped else TwoHandPlanAgent


class PopulationPlanAgent(BaseAgent):
    """One ``HandPlanAgent`` per env, each with weights of its own, all searched in one launch per move
    (``bb_plan_actions_each``).  ``rows``: int32 [N, 8], env i's weights in the order of ``L.GREEDY_FIELDS``
    (``runtime.kernels.weight_rows`` makes them from dicts), or int32 [N, 12] in the order of ``L.EVAL_FIELDS``
    (``eval_rows``), which are searched with the shape terms by ``bb_plan_actions_ext`` at depth 1..3; they are moved
    to the agent's device.  ``depth`` 1..3
    is the search depth; ``depth=0`` asks for the one-ply greedy kernel (``bb_greedy_actions_each``), which chooses
    what depth 1 chooses.  Only ``act_env`` is offered: the agent is tied to a ``DeviceEnvBatch`` of N envs
    (``evaluation/tune.py`` plays a population of candidate weights with it)."""

    def __init__(self, rows: torch.Tensor, depth: int = 3, device=None):
        from runtime.device_env import resolve_device

        super().__init__(resolve_device(device))
        if int(depth) not in (0, 1, 2, 3):
            raise ValueError(f"depth must be 0 (the one-ply greedy kernel), 1, 2 or 3, not {depth}")
        self.depth = int(depth)
        self.rows = rows.to(self.device).contiguous()
        self.ext = self.rows.dim() == 2 and self.rows.shape[1] == len(L.EVAL_FIELDS)
        if self.ext and self.depth == 0:
            raise ValueError("rows of twelve weights need depth 1..3: the one-ply greedy kernel has no extended form")

    def act_env(self, env_batch, out: torch.Tensor) -> torch.Tensor:
        if self.ext:
            return env_batch.plan_actions_ext(out, self.rows, self.depth)
        if self.depth == 0:
            return env_batch.greedy_actions_each(out, self.rows)
        return env_batch.plan_actions_each(out, self.rows, self.depth)

    def select_action(self, observation: Dict[str, Any], deterministic: bool = True) -> Tuple[int, Dict[str, Any]]:
        raise NotImplementedError("PopulationPlanAgent plays a DeviceEnvBatch (act_env); for one game use HandPlanAgent")

    def update(self, *args, **kwargs) -> Dict[str, float]:
        return {}

    def save(self, path: str) -> None:
        raise NotImplementedError("a population has no single weights file; save the HandPlanAgent of one row")

    def load(self, path: str) -> None:
        raise NotImplementedError("a population has no single weights file; load a HandPlanAgent")


class PopulationTwoHandAgent(BaseAgent):
    """One two-hand agent per env, each with weights of its own, decided in one ``bb_plan2_values`` call per move: no
    host read, no torch arithmetic, one cached workspace.  ``rows``: int32 [N, 12] (or [1, 12] for one shared set) in
    the order of ``L.EVAL_FIELDS`` (``runtime.kernels.eval_rows``); they are moved to the agent's device.  ``stream``:
    int64 [N] stream ids of the deals (None: env i draws from stream i); envs given the same id meet the same dealt
    hands.  The deals of move t are keyed by ``TwoHandPlanAgent.deal_seed(seed, t)``.  With every row equal to one
    weight set and ``stream=None`` it plays move for move what ``two_hand_agent_class(w)(w, depth, candidates, deals,
    seed)`` plays.  Only ``act_env`` is offered, as with ``PopulationPlanAgent``."""

    def __init__(self, rows: torch.Tensor, depth: int = 3, candidates: int = 8, deals: int = 16, seed: int = 0,
                 stream: Optional[torch.Tensor] = None, device=None):
        from runtime.device_env import resolve_device

        super().__init__(resolve_device(device))
        if int(depth) not in (1, 2, 3):
            raise ValueError(f"depth must be 1, 2 or 3, not {depth}")
        if not 1 <= int(candidates) <= 192:
            raise ValueError(f"candidates must be 1..192, not {candidates}")
        if not 1 <= int(deals) <= L.BB_REFILL_MAX_DEALS:
            raise ValueError(f"deals must be 1..{L.BB_REFILL_MAX_DEALS}, not {deals}")
        if not (isinstance(rows, torch.Tensor) and rows.dim() == 2 and rows.shape[1] == len(L.EVAL_FIELDS)):
            raise ValueError(f"rows must be an int32 [N, {len(L.EVAL_FIELDS)}] tensor (runtime.kernels.eval_rows)")
        self.depth, self.candidates, self.deals, self.seed = int(depth), int(candidates), int(deals), int(seed)
        self.rows = rows.to(self.device).contiguous()
        self.stream = None if stream is None else stream.to(self.device).contiguous()
        self.moves = 0  # decisions made so far: mixed into the deals' seed
        self._work = None

    def act_env(self, env_batch, out: torch.Tensor) -> torch.Tensor:
        """The action of every env of a ``DeviceEnvBatch`` into out (int32 [N]); one decision of the move counter."""
        from runtime import kernels as K

        if self._work is None or self._work[0] != env_batch.num_envs or self._work[1].device != env_batch.device:
            need = K.plan2_work_bytes(env_batch.num_envs, self.candidates, self.deals,
                                      host=env_batch.device.type == "cpu")
            self._work = (env_batch.num_envs, torch.empty(max(need, 8), dtype=torch.uint8, device=env_batch.device))
        env_batch.plan2_values(self.rows, self.candidates, self.deals, TwoHandPlanAgent.deal_seed(self.seed, self.moves),
                               stream=self.stream, depth=self.depth, out={"action": out}, work=self._work[1])
        self.moves += 1
        return out

    def select_action(self, observation: Dict[str, Any], deterministic: bool = True) -> Tuple[int, Dict[str, Any]]:
        raise NotImplementedError("PopulationTwoHandAgent plays a DeviceEnvBatch (act_env); for one game use "
                                  "TwoHandPlanAgent / TwoHandShapeAgent")

    def update(self, *args, **kwargs) -> Dict[str, float]:
        return {}

    def save(self, path: str) -> None:
        raise NotImplementedError("a population has no single weights file; save the TwoHandPlanAgent of one row")

    def load(self, path: str) -> None:
        raise NotImplementedError("a population has no single weights file; load a TwoHandPlanAgent")


class RandomAgent(BaseAgent):
    """Uniform random legal play: the Philox policy of ``bb_random_actions`` (bb_step_out.next_action), keyed
    by ``seed`` and counting one step per call.  ``safe=True`` (``act_env`` only) draws from the hand-safe actions
    of ``bb_plan_values`` instead -- the legal moves after which the rest of the hand still fits in some order -- and
    from the legal ones where no move is safe: such a player never loses in the middle of a hand."""

    def __init__(self, seed: int = 0xB10C, device=None, safe: bool = False):
        from runtime.device_env import resolve_device

        super().__init__(resolve_device(device))
        self.seed = int(seed)
        self.step = 0
        self.safe = bool(safe)
        self._mask_bits = None
        self._safe_bits = None

    def act_env(self, env_batch, out: torch.Tensor) -> torch.Tensor:
        n = env_batch.num_envs
        if self._mask_bits is None or self._mask_bits.shape[0] != n or self._mask_bits.device != env_batch.device:
            self._mask_bits = torch.zeros((n, 3), dtype=torch.int64, device=env_batch.device)
            self._safe_bits = torch.zeros_like(self._mask_bits)
        env_batch.obs(mask_bits=self._mask_bits)
        if self.safe:
            apply_safe_mask(env_batch, self._mask_bits, self._safe_bits)
        env_batch.random_actions(self._mask_bits, out, seed=self.seed, step=self.step)
        self.step += 1
        return out

    def select_action(self, observation: Dict[str, Any], deterministic: bool = False) -> Tuple[int, Dict[str, Any]]:
        from runtime import kernels as K
        from runtime.device_env import _ptr, _stream

        mask = torch.as_tensor(np.asarray(observation["action_mask"]).reshape(1, 3, 64) != 0)
        bits = (mask.to(torch.int64) << torch.arange(64)).sum(-1).to(self.device).contiguous()
        out = torch.zeros(1, dtype=torch.int32, device=self.device)
        lib, _ = K._look_lib(self.device)
        L.check(lib.bb_random_actions(_ptr(bits), 1, self.seed, self.step, 0, _ptr(out), _stream(self.device)),
                "bb_random_actions", lib=lib)
        self.step += 1
        return int(out.cpu().item()), {}

    def update(self, *args, **kwargs) -> Dict[str, float]:
        return {}

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump({"agent": "random", "seed": self.seed}, f, indent=2)

    def load(self, path: str) -> None:
        with open(path) as f:
            self.seed = int(json.load(f)["seed"])
