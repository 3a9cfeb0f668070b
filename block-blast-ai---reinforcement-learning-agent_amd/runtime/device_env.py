"""Device-resident batch of Block Blast envs: one libbbvec handle + its buffers.

This is the torch-facing layer under the Gym surface.  All tensors live on the
handle's GPU; every call launches on torch's current stream of that device and
never synchronises (except the explicit host copies ``state()`` /
``set_state()``).

``device="cpu"`` selects the host backend (libbbvec_host.so, the same C-ABI on
CPU tensors, csrc/bb_host.cpp) explicitly; without it a missing HIP device is
an error, never a silent switch to the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L

DEFAULT_REWARDS = {  # block_blast_env.py:63-71
    "line_clear_base": 1.0,
    "block_placed": 0.01,
    "game_over_penalty": -1.0,
    "hole_penalty": -0.05,
    "center_bonus": 0.02,
    "combo_multiplier_bonus": 0.5,
    "survival_bonus": 0.001,
}

INFO_DTYPE = np.dtype(
    [
        ("score", "<i8"), ("score_gained", "<i8"), ("term_board", "<u8"),
        ("moves", "<i4"), ("lines", "<i4"), ("max_combo", "<i4"), ("blocks", "<i4"),
        ("term_hand", "<u4"), ("holes", "u1"), ("filled", "u1"), ("flags", "u1"),
        ("last_blocks", "u1"), ("last_lines", "u1"), ("last_cm", "u1"), ("pad", "u1", (2,)),
    ],
    align=True,
)
assert INFO_DTYPE.itemsize == L.INFO_BYTES


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    if device.type == "cpu":
        return None
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def resolve_device(device=None) -> torch.device:
    if device is not None and torch.device(device).type == "cpu":  # the host backend, asked for by name
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise L.BBNativeError("no GPU visible to torch: the Block Blast env runs only on the HIP device")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device(device)
    if d.type != "cuda":
        raise L.BBNativeError(f"Block Blast env needs a cuda (HIP) device, got {d}")
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


def seeds_to_arrays(seeds: Sequence[Optional[int]]):
    """Per-env seeds (int or None) -> (seed u64, has_seed u8, raw u64[N,4])."""
    n = len(seeds)
    s = np.zeros(n, dtype=np.uint64)
    has = np.zeros(n, dtype=np.uint8)
    raw = np.zeros((n, 4), dtype=np.uint64)
    need_entropy = []
    for i, sd in enumerate(seeds):
        if sd is None:
            need_entropy.append(i)
            continue
        sd = int(sd)
        if sd < 0:
            raise ValueError("expected non-negative integer seed (numpy SeedSequence semantics)")
        if sd < 2 ** 64:
            s[i] = sd
            has[i] = 1
        else:  # does not fit the C-ABI's uint64: let numpy's SeedSequence do it
            st = np.random.PCG64(sd).state["state"]
            raw[i] = [st["state"] >> 64, st["state"] & (2 ** 64 - 1), st["inc"] >> 64, st["inc"] & (2 ** 64 - 1)]
            has[i] = 2
    if need_entropy:  # seed_value None: fresh OS entropy, stream continues across resets
        ent = np.random.default_rng().integers(0, 2 ** 63, size=(len(need_entropy), 4), dtype=np.int64)
        raw[need_entropy] = ent.astype(np.uint64)
    return s, has, raw


class DeviceEnvBatch:
    """``num_envs`` Block Blast games stepped in lockstep by ``bb_step``."""

    def __init__(
        self,
        num_envs: int,
        seeds: Optional[Sequence[Optional[int]]] = None,
        reward_config: Optional[dict] = None,
        autoreset: bool = True,
        device=None,
        env_offset: int = 0,
    ):
        self.device = resolve_device(device)
        self.lib = L.load_host() if self.device.type == "cpu" else L.load()
        self.num_envs = int(num_envs)
        self.env_offset = int(env_offset)
        rw = dict(DEFAULT_REWARDS)
        if reward_config:
            rw.update(reward_config)
        self.reward_config = rw
        h = C.c_void_p()
        L.check(
            self.lib.bb_create(self.num_envs, self.device.index or 0, C.byref(L.reward_cfg(rw)), int(bool(autoreset)),
                               C.byref(h)),
            "bb_create", lib=self.lib,
        )
        self.handle = h
        dev = self.device
        n = self.num_envs
        self.reward = torch.zeros(n, dtype=torch.float32, device=dev)
        self.terminated = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.reward_f64 = torch.zeros(n, dtype=torch.float64, device=dev)
        self.lines = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.info = torch.zeros(n * L.INFO_BYTES, dtype=torch.uint8, device=dev)
        self._out = L.StepOut()
        self.seed(seeds if seeds is not None else [None] * n)

    # ------------------------------------------------------------------ seeding
    def seed(self, seeds: Sequence[Optional[int]]) -> None:
        if len(seeds) != self.num_envs:
            raise ValueError("one seed (or None) per env expected")
        s, has, raw = seeds_to_arrays(seeds)
        L.check(
            self.lib.bb_seed(self.handle, s.ctypes.data_as(C.c_void_p), has.ctypes.data_as(C.c_void_p),
                             raw.ctypes.data_as(C.c_void_p)),
            "bb_seed", self.handle, self.lib,
        )

    # --------------------------------------------------------------- hot path
    def reset(self, env_mask: Optional[torch.Tensor] = None) -> None:
        L.check(self.lib.bb_reset(self.handle, _ptr(env_mask), _stream(self.device)), "bb_reset", self.handle, self.lib)

    def step(
        self,
        actions: torch.Tensor,
        want_info: bool = False,
        want_f64: bool = False,
        want_lines: bool = False,
        next_action: Optional[torch.Tensor] = None,
        policy_seed: int = 0xB10C,
        policy_step: int = 0,
        mask_out: Optional[torch.Tensor] = None,
        final_score: Optional[torch.Tensor] = None,
        final_moves: Optional[torch.Tensor] = None,
    ) -> None:
        """actions: int32 [N] on this device.  Outputs land in self.reward /
        self.terminated (+ reward_f64 / lines / info when requested).
        final_score (int64 [N]) / final_moves (int32 [N]) receive the score and
        moves of the envs that terminated (info['final_score'] / info['moves'])
        and are left untouched elsewhere."""
        assert actions.dtype == torch.int32 and actions.device == self.device and actions.numel() == self.num_envs
        for t, dt in ((final_score, torch.int64), (final_moves, torch.int32)):
            assert t is None or (t.dtype == dt and t.device == self.device and t.is_contiguous() and t.numel() == self.num_envs)
        o = self._out
        o.reward = self.reward.data_ptr()
        o.terminated = self.terminated.data_ptr()
        o.reward_f64 = self.reward_f64.data_ptr() if want_f64 else None
        o.mask = mask_out.data_ptr() if mask_out is not None else None
        o.lines = self.lines.data_ptr() if want_lines else None
        o.info = self.info.data_ptr() if want_info else None
        o.next_action = next_action.data_ptr() if next_action is not None else None
        o.policy_seed = policy_seed
        o.policy_step = policy_step
        o.env_offset = self.env_offset
        o.final_score = final_score.data_ptr() if final_score is not None else None
        o.final_moves = final_moves.data_ptr() if final_moves is not None else None
        L.check(self.lib.bb_step(self.handle, _ptr(actions), C.byref(o), _stream(self.device)), "bb_step",
                self.handle, self.lib)

    def rollout(
        self,
        steps: int,
        actions: torch.Tensor,
        reward: torch.Tensor,
        terminated: torch.Tensor,
        lines: Optional[torch.Tensor] = None,
        actions_out: Optional[torch.Tensor] = None,
        mask_out: Optional[torch.Tensor] = None,
        next_action: Optional[torch.Tensor] = None,
        policy_seed: int = 0xB10C,
        policy_step0: int = 0,
    ) -> None:
        """``steps`` fused steps under the synthetic random policy (bb_rollout).
        actions: int32 [N], the action of the first step; reward f32 / terminated
        u8 / lines u8 / actions_out i32 are [steps, N], mask_out i64 [steps, N, 3].
        Equals ``steps`` chained ``step(..., next_action=, policy_step=policy_step0+t+1)``."""
        n = self.num_envs
        assert actions.dtype == torch.int32 and actions.device == self.device and actions.numel() == n
        assert reward.dtype == torch.float32 and reward.numel() >= steps * n
        assert terminated.dtype == torch.uint8 and terminated.numel() >= steps * n
        for t, dt, per in ((lines, torch.uint8, 1), (actions_out, torch.int32, 1), (mask_out, torch.int64, 3),
                           (next_action, torch.int32, 0)):
            if t is not None:
                assert t.dtype == dt and t.device == self.device and t.numel() >= (steps * n * per if per else n)
        o = L.RolloutOut(reward=reward.data_ptr(), terminated=terminated.data_ptr(),
                         lines=lines.data_ptr() if lines is not None else None,
                         actions=actions_out.data_ptr() if actions_out is not None else None,
                         mask=mask_out.data_ptr() if mask_out is not None else None,
                         next_action=next_action.data_ptr() if next_action is not None else None,
                         policy_seed=policy_seed, policy_step0=policy_step0, env_offset=self.env_offset)
        L.check(self.lib.bb_rollout(self.handle, int(steps), _ptr(actions), C.byref(o), _stream(self.device)),
                "bb_rollout", self.handle, self.lib)

    def sync(self) -> None:
        """Wait for this handle's launches on the current stream and raise BBNativeError if a kernel reported
        a device-side failure (bb_sync; e.g. a rollout wave that hit its iteration cap)."""
        L.check(self.lib.bb_sync(self.handle, _stream(self.device)), "bb_sync", self.handle, self.lib)

    def obs(self, x=None, mask_i8=None, mask_f32=None, mask_bits=None) -> None:
        L.check(
            self.lib.bb_obs(self.handle, _ptr(x), _ptr(mask_i8), _ptr(mask_f32), _ptr(mask_bits),
                            _stream(self.device)),
            "bb_obs", self.handle, self.lib,
        )

    def snapshot(self, board=None, hand=None, mask_bits=None) -> None:
        L.check(
            self.lib.bb_snapshot(self.handle, _ptr(board), _ptr(hand), _ptr(mask_bits), _stream(self.device)),
            "bb_snapshot", self.handle, self.lib,
        )

    def snapshot_combo(self, out: torch.Tensor) -> None:
        """bb_snapshot_combo: the live combo column into out (int32 [N]); with ``snapshot``'s board and hand a
        stored position that ``runtime.kernels.plan_values`` can search later."""
        assert out.dtype == torch.int32 and out.device == self.device and out.is_contiguous() \
            and out.numel() == self.num_envs
        L.check(self.lib.bb_snapshot_combo(self.handle, _ptr(out), _stream(self.device)), "bb_snapshot_combo",
                self.handle, self.lib)

    def random_actions(self, mask_bits: torch.Tensor, out: torch.Tensor, seed: int = 0xB10C, step: int = 0):
        L.check(
            self.lib.bb_random_actions(_ptr(mask_bits), self.num_envs, seed, step, self.env_offset, _ptr(out),
                                       _stream(self.device)),
            "bb_random_actions", None, self.lib,
        )

    # ------------------------------------------------------------ lookahead
    def afterstates(self, out: Optional[dict] = None) -> dict:
        """bb_afterstates on the live state: for each of the 192 actions of every env the board it leads to,
        its fp64 reward, its score and the packed aux word (bbvec.h), [N, 192] each.  ``out``: a dict with any
        of "board" i64, "reward" f64, "score_gained" i32, "aux" i32 tensors to write (missing = not computed);
        None = all four, freshly allocated.  Reads the state and changes nothing, the piece stream included."""
        from . import kernels as K

        out = K.afterstate_outputs(self.num_envs, self.device) if out is None else out
        o = K._afterstate_out(out, self.num_envs, self.device)
        L.check(self.lib.bb_afterstates(self.handle, C.byref(o), _stream(self.device)), "bb_afterstates",
                self.handle, self.lib)
        return out

    def greedy_actions(self, out: torch.Tensor, weights, value: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bb_greedy_actions on the live state: out (int32 [N]) receives every env's best legal action under
        the one-ply greedy value of ``weights`` (a dict of bb_greedy_weights fields or an L.GreedyWeights), ties
        to the lowest action, 0 where nothing is legal; value (int64 [N], optional) that value."""
        from . import kernels as K

        n = self.num_envs
        for t, dt in ((out, torch.int32), (value, torch.int64)):
            assert t is None or (t.dtype == dt and t.device == self.device and t.is_contiguous() and t.numel() == n)
        w = K._weights(weights)
        L.check(self.lib.bb_greedy_actions(self.handle, C.byref(w), _ptr(out), _ptr(value), _stream(self.device)),
                "bb_greedy_actions", self.handle, self.lib)
        return out

    def plan_actions(self, out: torch.Tensor, weights, depth: int = 3, value: Optional[torch.Tensor] = None,
                     plan: Optional[torch.Tensor] = None, leaves: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bb_plan_actions on the live state: out (int32 [N]) receives the first move of every env's best way
        to play out its hand, searched exhaustively up to ``depth`` (1..3) moves in one fused launch; value
        (int64 [N]), plan (int32 [N, 3], -1 for plies not played) and leaves (int32 [N], the number of maximal
        sequences) are optional.  Reads the state and changes nothing, the piece stream included."""
        from . import kernels as K

        o = K._plan_out({"action": out, "value": value, "plan": plan, "leaves": leaves}, self.num_envs, self.device)
        w = K._weights(weights)
        L.check(self.lib.bb_plan_actions(self.handle, C.byref(w), int(depth), C.byref(o), _stream(self.device)),
                "bb_plan_actions", self.handle, self.lib)
        return out

    def greedy_actions_each(self, out: torch.Tensor, rows: torch.Tensor,
                            value: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bb_greedy_actions_each on the live state: ``greedy_actions`` with env i's weights taken from rows[i]
        (int32 [N, 8] on this device, ``runtime.kernels.weight_rows``), read when the launch runs."""
        from . import kernels as K

        n = self.num_envs
        for t, dt in ((out, torch.int32), (value, torch.int64)):
            assert t is None or (t.dtype == dt and t.device == self.device and t.is_contiguous() and t.numel() == n)
        K._rows("greedy_actions_each", rows, n, self.device)
        L.check(self.lib.bb_greedy_actions_each(self.handle, _ptr(rows), _ptr(out), _ptr(value),
                                                _stream(self.device)),
                "bb_greedy_actions_each", self.handle, self.lib)
        return out

    def plan_actions_each(self, out: torch.Tensor, rows: torch.Tensor, depth: int = 3,
                          value: Optional[torch.Tensor] = None, plan: Optional[torch.Tensor] = None,
                          leaves: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bb_plan_actions_each on the live state: ``plan_actions`` with env i's weights taken from rows[i] (int32
        [N, 8] on this device, ``runtime.kernels.weight_rows``), read when the launch runs: one launch searches for
        a whole population of weight vectors."""
        from . import kernels as K

        o = K._plan_out({"action": out, "value": value, "plan": plan, "leaves": leaves}, self.num_envs, self.device)
        K._rows("plan_actions_each", rows, self.num_envs, self.device)
        L.check(self.lib.bb_plan_actions_each(self.handle, _ptr(rows), int(depth), C.byref(o), _stream(self.device)),
                "bb_plan_actions_each", self.handle, self.lib)
        return out

    def board_terms(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bb_board_terms on the live boards: int32 [N, 4], the shape terms in the order of ``L.TERM_FIELDS``
        (perimeter, room3, room5, fits)."""
        n = self.num_envs
        out = torch.empty((n, 4), dtype=torch.int32, device=self.device) if out is None else out
        assert out.dtype == torch.int32 and out.device == self.device and out.is_contiguous() and out.numel() == n * 4
        L.check(self.lib.bb_board_terms(self.handle, _ptr(out), _stream(self.device)), "bb_board_terms", self.handle,
                self.lib)
        return out

    def plan_actions_ext(self, out: torch.Tensor, rows: torch.Tensor, depth: int = 3,
                         value: Optional[torch.Tensor] = None, plan: Optional[torch.Tensor] = None,
                         leaves: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bb_plan_actions_ext on the live state: ``plan_actions`` with the shape terms in every leaf's value.  rows:
        int32 [1, 12] (one row for all envs) or [N, 12] on this device (``runtime.kernels.eval_rows``), read when the
        launch runs."""
        from . import kernels as K

        o = K._plan_out({"action": out, "value": value, "plan": plan, "leaves": leaves}, self.num_envs, self.device)
        stride = K._eval_rows("plan_actions_ext", rows, self.num_envs, self.device)
        L.check(self.lib.bb_plan_actions_ext(self.handle, _ptr(rows), stride, int(depth), C.byref(o),
                                             _stream(self.device)),
                "bb_plan_actions_ext", self.handle, self.lib)
        return out

    def plan_values(self, weights, depth: int = 3, out: Optional[dict] = None) -> dict:
        """bb_plan_values on the live state: the search of ``plan_actions`` kept per first move.  ``out``: a dict
        with any of "q" i64 / "rest" i32 / "leaves" i32 [N, 192] and "safe" i64 [N, 3] tensors to write (missing
        = not computed); None = all four, freshly allocated (see ``runtime.kernels.plan_values``).  Reads the
        state and changes nothing, the piece stream included."""
        from . import kernels as K

        out = K.plan_value_outputs(self.num_envs, self.device) if out is None else out
        o = K._plan_values_out(out, self.num_envs, self.device)
        w = K._weights(weights)
        L.check(self.lib.bb_plan_values(self.handle, C.byref(w), int(depth), C.byref(o), _stream(self.device)),
                "bb_plan_values", self.handle, self.lib)
        return out

    def safe_mask(self, out: torch.Tensor, depth: int = 3) -> torch.Tensor:
        """The hand-safe action mask into out (int64 [N, 3], the layout of ``obs(mask_bits=)``): the legal actions
        after which the rest of the hand can still be placed in some order.  All zeros where no legal action is
        safe (or none is legal).  One launch, nothing else written.  depth >= 2: bb_safe_mask, the existence
        search; depth 1 (legal & !dead, another set): bb_plan_values."""
        if int(depth) in (2, 3):  # any other depth is bb_plan_values' to answer or refuse
            return self._safe_mask(0, out)
        self.plan_values({}, depth, out={"safe": out})
        return out

    def sampling_mask(self, out: torch.Tensor) -> torch.Tensor:
        """The mask to sample under when training or playing hand-safe, into out (int64 [N, 3]): an env's safe words
        (``safe_mask`` at depth >= 2) where it has a safe action, else its legal words (all zeros for a finished
        game).  One launch (bb_safe_mask, mode BB_SAFE_OR_LEGAL); reads the state and changes nothing."""
        return self._safe_mask(1, out)

    def _safe_mask(self, mode: int, out: torch.Tensor) -> torch.Tensor:
        from . import kernels as K

        K._safe_mask_out(out, self.num_envs, self.device)
        L.check(self.lib.bb_safe_mask(self.handle, int(mode), _ptr(out), _stream(self.device)), "bb_safe_mask",
                self.handle, self.lib)
        return out

    def refill_census(self, count: Optional[torch.Tensor] = None, solvable: Optional[torch.Tensor] = None) -> dict:
        """bb_refill_census on the live boards: count (int32 [N]) receives the number of the 37^3 ordered hands that
        can still be placed on each env's board in some order, solvable (int64 [N, 37, 37]) the hands themselves (bit
        c of word [a, b]).  Both None: a fresh count.  Returns the dict of what was written.  Reads the board column
        and changes nothing, the piece stream included (see ``runtime.kernels.refill_census``)."""
        from . import kernels as K

        out = {k: t for k, t in (("count", count), ("solvable", solvable)) if t is not None}
        out = out or K.census_outputs(self.num_envs, self.device)
        o = K._census_out(out, self.num_envs, self.device)
        L.check(self.lib.bb_refill_census(self.handle, C.byref(o), _stream(self.device)), "bb_refill_census",
                self.handle, self.lib)
        return out

    def refill_values(self, weights, deals: int, seed: int, stream: Optional[torch.Tensor] = None, depth: int = 3,
                      want=("value",), out: Optional[dict] = None) -> dict:
        """bb_refill_values on the live boards and combos: ``deals`` next hands per env dealt by the reference
        dealer's law and each searched (see ``runtime.kernels.refill_values``): a dict of [N, deals] tensors, "hand"
        int32, "value" int64, "attempts" int32, those named in ``want`` or given in ``out``.  stream int64 [N] or
        None (the env's index).  Reads the state and changes nothing, the piece stream included."""
        from . import kernels as K

        K._refill_column("stream", stream, torch.int64, self.num_envs, self.device)
        out, o = K._refill_values_args(deals, depth, out, self.num_envs, self.device, want)
        w = K._weights(weights)
        L.check(self.lib.bb_refill_values(self.handle, _ptr(stream), C.byref(w), depth, deals,
                                          int(seed) & (2 ** 64 - 1), C.byref(o), _stream(self.device)),
                "bb_refill_values", self.handle, self.lib)
        return out

    def plan_values_ext(self, rows: torch.Tensor, depth: int = 3, out: Optional[dict] = None) -> dict:
        """bb_plan_values_ext on the live state: ``plan_values`` with the shape terms in every sequence's value.
        rows: int32 [1, 12] (one row for all envs) or [N, 12] on this device (``runtime.kernels.eval_rows``), read
        when the launch runs.  ``out`` as ``plan_values``.  Reads the state and changes nothing."""
        from . import kernels as K

        out = K.plan_value_outputs(self.num_envs, self.device) if out is None else out
        o = K._plan_values_out(out, self.num_envs, self.device)
        stride = K._eval_rows("plan_values_ext", rows, self.num_envs, self.device)
        L.check(self.lib.bb_plan_values_ext(self.handle, _ptr(rows), stride, int(depth), C.byref(o),
                                            _stream(self.device)),
                "bb_plan_values_ext", self.handle, self.lib)
        return out

    def refill_values_ext(self, rows: torch.Tensor, deals: int, seed: int, stream: Optional[torch.Tensor] = None,
                          depth: int = 3, want=("value",), out: Optional[dict] = None) -> dict:
        """bb_refill_values_ext on the live boards and combos: ``refill_values`` with the shape terms in every dealt
        hand's value, every deal of env i under rows[i] (or the one shared row).  Reads the state and changes
        nothing, the piece stream included."""
        from . import kernels as K

        K._refill_column("stream", stream, torch.int64, self.num_envs, self.device)
        out, o = K._refill_values_args(deals, depth, out, self.num_envs, self.device, want)
        stride = K._eval_rows("refill_values_ext", rows, self.num_envs, self.device)
        L.check(self.lib.bb_refill_values_ext(self.handle, _ptr(stream), _ptr(rows), stride, depth, deals,
                                              int(seed) & (2 ** 64 - 1), C.byref(o), _stream(self.device)),
                "bb_refill_values_ext", self.handle, self.lib)
        return out

    def plan2_values(self, rows: torch.Tensor, candidates: int, deals: int, seed: int,
                     stream: Optional[torch.Tensor] = None, depth: int = 3, want=("action",),
                     out: Optional[dict] = None, work: Optional[torch.Tensor] = None) -> dict:
        """bb_plan2_values on the live boards, hands and combos: the two-hand decision of every env in one
        asynchronous call with no host read (``runtime.kernels.plan2_values`` names the steps and the outputs), env i
        under rows[i] (or the one shared row) and stream id ``stream[i]`` (or i).  ``work``: uint8 scratch of at least
        ``kernels.plan2_work_bytes(num_envs, candidates, deals)`` bytes on the env's device, allocated when None.
        Reads the state and changes nothing, the piece stream included."""
        from . import kernels as K

        n = self.num_envs
        K._refill_column("stream", stream, torch.int64, n, self.device)
        stride = K._eval_rows("plan2_values", rows, n, self.device)
        out, o, work, _ = K._plan2_args("plan2_values", self.lib, n, self.device, candidates, deals, depth, want, out,
                                        work)
        L.check(self.lib.bb_plan2_values(self.handle, _ptr(stream), _ptr(rows), stride, depth, candidates, deals,
                                         int(seed) & (2 ** 64 - 1), _ptr(work), work.numel(), C.byref(o),
                                         _stream(self.device)),
                "bb_plan2_values", self.handle, self.lib)
        return out

    def playout_values(self, rows: torch.Tensor, playouts: int, hands: int, seed: int,
                       stream: Optional[torch.Tensor] = None, depth: int = 3, want=("value",),
                       out: Optional[dict] = None) -> dict:
        """bb_playout_values on the live boards and combos: ``playouts`` dealt playouts of ``hands`` hands per env in
        one launch (``runtime.kernels.playout_values`` names the steps and the outputs), every playout of env i under
        rows[i] (or the one shared row) and stream id ``stream[i]`` (or i).  Reads the state and changes nothing, the
        piece stream included."""
        from . import kernels as K

        K._refill_column("stream", stream, torch.int64, self.num_envs, self.device)
        out, o = K._playout_args(playouts, hands, depth, out, self.num_envs, self.device, want)
        stride = K._eval_rows("playout_values", rows, self.num_envs, self.device)
        L.check(self.lib.bb_playout_values(self.handle, _ptr(stream), _ptr(rows), stride, depth, playouts, hands,
                                           int(seed) & (2 ** 64 - 1), C.byref(o), _stream(self.device)),
                "bb_playout_values", self.handle, self.lib)
        return out

    # ------------------------------------------------------------ host copies
    def state(self) -> dict:
        n = self.num_envs
        out = {
            "board": np.zeros(n, np.uint64), "hand": np.zeros(n, np.uint32), "score": np.zeros(n, np.int64),
            "combo": np.zeros(n, np.int32), "max_combo": np.zeros(n, np.int32), "moves": np.zeros(n, np.int32),
            "lines": np.zeros(n, np.int32), "blocks": np.zeros(n, np.int32), "prev_holes": np.zeros(n, np.uint8),
            "prev_center": np.zeros(n, np.uint8), "rng": np.zeros((n, 3), np.uint64),
        }
        v = L.StateView(**{k: a.ctypes.data for k, a in out.items()})
        L.check(self.lib.bb_get_state(self.handle, C.byref(v)), "bb_get_state", self.handle, self.lib)
        return out

    def set_state(self, **arrays) -> None:
        dt = {"board": np.uint64, "hand": np.uint32, "score": np.int64, "combo": np.int32, "max_combo": np.int32,
              "moves": np.int32, "lines": np.int32, "blocks": np.int32, "prev_holes": np.uint8,
              "prev_center": np.uint8, "rng": np.uint64}
        keep = {}
        kw = {}
        for k, a in arrays.items():
            arr = np.ascontiguousarray(a, dtype=dt[k])
            keep[k] = arr
            kw[k] = arr.ctypes.data
        v = L.StateView(**kw)
        L.check(self.lib.bb_set_state(self.handle, C.byref(v)), "bb_set_state", self.handle, self.lib)

    def info_host(self) -> np.ndarray:
        return self.info.cpu().numpy().view(INFO_DTYPE)

    def close(self) -> None:
        if getattr(self, "handle", None):
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self.lib.bb_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
