"""ctypes binding of ``include/bbvec.h`` (libbbvec.so, gfx950).

This is the only way the product reaches its kernels.  There is no CPU
fallback: if the library is missing or no HIP device is present, the first
call raises ``BBNativeError`` with the reason.

``load_host()`` binds the env half of the same ABI from libbbvec_host.so, the
host backend (csrc/bb_host.cpp) that ``DeviceEnvBatch(device="cpu")`` selects
explicitly; nothing falls back to it.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("BBVEC_LIB", os.path.join(PKG_DIR, "libbbvec.so"))
HOST_LIB_PATH = os.path.join(PKG_DIR, "libbbvec_host.so")

BB_OK = 0
BB_ACTIONS = 192
BB_NUM_PIECES = 37
BB_NUM_HANDS = 50653  # 37^3 ordered hands
BB_REFILL_MAX_DEALS = 1024
BB_PLAYOUT_MAX_HANDS = 256
BB_PLAY_PLIES, BB_PLAY_DEAD, BB_PLAY_REFILL, BB_PLAY_ILLEGAL = 3, 4, 8, 16  # bb_play_plan_out.status


class BBNativeError(RuntimeError):
    """Raised when the HIP library is unavailable or a C-ABI call fails."""


class RewardCfg(C.Structure):
    _fields_ = [
        ("line_clear_base", C.c_double),
        ("block_placed", C.c_double),
        ("game_over_penalty", C.c_double),
        ("hole_penalty", C.c_double),
        ("center_bonus", C.c_double),
        ("combo_multiplier_bonus", C.c_double),
        ("survival_bonus", C.c_double),
    ]


class Info(C.Structure):
    _fields_ = [
        ("score", C.c_int64),
        ("score_gained", C.c_int64),
        ("term_board", C.c_uint64),
        ("moves", C.c_int32),
        ("lines", C.c_int32),
        ("max_combo", C.c_int32),
        ("blocks", C.c_int32),
        ("term_hand", C.c_uint32),
        ("holes", C.c_uint8),
        ("filled", C.c_uint8),
        ("flags", C.c_uint8),
        ("last_blocks", C.c_uint8),
        ("last_lines", C.c_uint8),
        ("last_cm", C.c_uint8),
        ("pad", C.c_uint8 * 2),
    ]


ABI_VERSION = 9  # include/bbvec.h BB_ABI_VERSION
INFO_BYTES = C.sizeof(Info)  # 56, matches sizeof(bb_info)


class StepOut(C.Structure):
    _fields_ = [
        ("reward", C.c_void_p),
        ("terminated", C.c_void_p),
        ("reward_f64", C.c_void_p),
        ("mask", C.c_void_p),
        ("lines", C.c_void_p),
        ("info", C.c_void_p),
        ("next_action", C.c_void_p),
        ("policy_seed", C.c_uint64),
        ("policy_step", C.c_uint64),
        ("env_offset", C.c_uint64),
        ("final_score", C.c_void_p),
        ("final_moves", C.c_void_p),
    ]


class RolloutOut(C.Structure):
    _fields_ = [
        ("reward", C.c_void_p),
        ("terminated", C.c_void_p),
        ("lines", C.c_void_p),
        ("actions", C.c_void_p),
        ("mask", C.c_void_p),
        ("next_action", C.c_void_p),
        ("policy_seed", C.c_uint64),
        ("policy_step0", C.c_uint64),
        ("env_offset", C.c_uint64),
    ]


class StateView(C.Structure):
    _fields_ = [
        ("board", C.c_void_p),
        ("hand", C.c_void_p),
        ("score", C.c_void_p),
        ("combo", C.c_void_p),
        ("max_combo", C.c_void_p),
        ("moves", C.c_void_p),
        ("lines", C.c_void_p),
        ("blocks", C.c_void_p),
        ("prev_holes", C.c_void_p),
        ("prev_center", C.c_void_p),
        ("rng", C.c_void_p),
    ]


class Positions(C.Structure):
    """bb_positions: device columns [n]; combo / prev may be NULL (= 0)."""
    _fields_ = [("board", C.c_void_p), ("hand", C.c_void_p), ("combo", C.c_void_p), ("prev", C.c_void_p)]


class AfterstateOut(C.Structure):
    """bb_afterstate_out: device arrays [n][192], any may be NULL."""
    _fields_ = [("board", C.c_void_p), ("reward_f64", C.c_void_p), ("score_gained", C.c_void_p), ("aux", C.c_void_p)]


GREEDY_FIELDS = ("lines", "score", "holes", "filled", "centre", "mobility", "dead", "refill")


class GreedyWeights(C.Structure):
    """bb_greedy_weights: the eight int32 weights of the one-ply greedy value."""
    _fields_ = [(k, C.c_int32) for k in GREEDY_FIELDS]


def greedy_weights(weights: dict) -> GreedyWeights:
    unknown = set(weights) - set(GREEDY_FIELDS)
    if unknown:
        raise ValueError(f"unknown greedy weights {sorted(unknown)}; the fields are {GREEDY_FIELDS}")
    return GreedyWeights(**{k: int(weights.get(k, 0)) for k in GREEDY_FIELDS})


# the shape terms of a board (bb_board_terms writes them in this order) and bb_eval_weights: the eight, then one
# weight per shape term
TERM_FIELDS = ("perimeter", "room3", "room5", "fits")
EVAL_FIELDS = GREEDY_FIELDS + TERM_FIELDS


class EvalWeights(C.Structure):
    """bb_eval_weights: bb_greedy_weights, then the four int32 weights of the shape terms (twelve int32)."""
    _fields_ = [("base", GreedyWeights)] + [(k, C.c_int32) for k in TERM_FIELDS]


def eval_weights(weights: dict) -> EvalWeights:
    unknown = set(weights) - set(EVAL_FIELDS)
    if unknown:
        raise ValueError(f"unknown evaluation weights {sorted(unknown)}; the fields are {EVAL_FIELDS}")
    return EvalWeights(base=greedy_weights({k: v for k, v in weights.items() if k in GREEDY_FIELDS}),
                       **{k: int(weights.get(k, 0)) for k in TERM_FIELDS})


class PlanOut(C.Structure):
    """bb_plan_out: device arrays action i32 [n] (required), value i64 [n], plan i32 [n][3], leaves i32 [n]."""
    _fields_ = [("action", C.c_void_p), ("value", C.c_void_p), ("plan", C.c_void_p), ("leaves", C.c_void_p)]


class PlanValuesOut(C.Structure):
    """bb_plan_values_out: device arrays q i64 / rest i32 / leaves i32 [n][192], safe u64 [n][3]; any may be NULL,
    not all four."""
    _fields_ = [("q", C.c_void_p), ("rest", C.c_void_p), ("leaves", C.c_void_p), ("safe", C.c_void_p)]


class CensusOut(C.Structure):
    """bb_census_out: device arrays count i32 [n], solvable u64 [n][37][37]; either may be NULL, not both."""
    _fields_ = [("count", C.c_void_p), ("solvable", C.c_void_p)]


class RefillValuesOut(C.Structure):
    """bb_refill_values_out: device arrays hand u32 / value i64 / attempts i32 [n][deals]; any may be NULL, not all."""
    _fields_ = [("hand", C.c_void_p), ("value", C.c_void_p), ("attempts", C.c_void_p)]


class Plan2Out(C.Structure):
    """bb_plan2_out: device arrays action i32 [n] / q2 i64 [n][192] / cand i32 [n][K] / status i32 [n][K] / value i64
    [n][K][deals]; any may be NULL, not all five."""
    _fields_ = [("action", C.c_void_p), ("q2", C.c_void_p), ("cand", C.c_void_p), ("status", C.c_void_p),
                ("value", C.c_void_p)]


class PlayoutOut(C.Structure):
    """bb_playout_out: device arrays value i64 / score i64 / lines i32 / plies i32 / hands i32 / status i32 / board
    u64 / combo i32 / hand u32, each [n][playouts]; any may be NULL, not all nine."""
    _fields_ = [("value", C.c_void_p), ("score", C.c_void_p), ("lines", C.c_void_p), ("plies", C.c_void_p),
                ("hands", C.c_void_p), ("status", C.c_void_p), ("board", C.c_void_p), ("combo", C.c_void_p),
                ("hand", C.c_void_p)]


class PlayPlanOut(C.Structure):
    """bb_play_plan_out: device arrays [n]; any may be NULL, not all six."""
    _fields_ = [("board", C.c_void_p), ("hand", C.c_void_p), ("combo", C.c_void_p), ("lines", C.c_void_p),
                ("score", C.c_void_p), ("status", C.c_void_p)]


_P = C.c_void_p
_I32 = C.c_int32
_U64 = C.c_uint64
_F = C.c_float


_BN_SHAPE = [("dtype", _I32), ("nhwc", _I32), ("N", _I32), ("C", _I32), ("HW", _I32)]


class BnFwd(C.Structure):
    """bb_bn_fwd: res, pre_bias, running_mean / _var, num_batches_tracked, part / nb_part are optional (NULL / 0)."""
    _fields_ = [("x", _P), ("res", _P), *_BN_SHAPE, ("pre_bias", _P), ("weight", _P), ("bias", _P), ("eps", _F),
                ("relu", _I32), ("ws", _P), ("save_mean", _P), ("save_invstd", _P), ("running_mean", _P),
                ("running_var", _P), ("momentum", _F), ("num_batches_tracked", _P), ("y", _P), ("part", _P),
                ("nb_part", _I32)]


class WgradReduce(C.Structure):
    """bb_wgrad_reduce: bb_conv3x3_wgrad_reduce's arguments; ws NULL = no job."""
    _fields_ = [("ws", _P), ("chunks", _I32), ("cin", _I32), ("cout", _I32), ("w_layout", _I32), ("dw", _P)]


class BnBwd(C.Structure):
    """bb_bn_bwd: y + gres (the ReLU mask of a residual tail), pre_bias, dweight / dbias / dpre_bias, reduce and
    part / nb_part are optional (NULL / 0)."""
    _fields_ = [("x", _P), ("dy", _P), ("y", _P), *_BN_SHAPE, ("pre_bias", _P), ("weight", _P), ("bias", _P),
                ("save_mean", _P), ("save_invstd", _P), ("relu", _I32), ("ws", _P), ("dx", _P), ("dweight", _P),
                ("dbias", _P), ("dpre_bias", _P), ("gres", _P), ("reduce", WgradReduce), ("part", _P),
                ("nb_part", _I32)]


class PpoLossArgs(C.Structure):
    """bb_ppo_loss_args: grad_loss / dlogits / dvalues are the backward's, ws / cnt / stats / loss the forward's."""
    _fields_ = [("logits", _P), ("values", _P), ("bf16", _I32), ("mask", _P), ("actions", _P), ("old_logp", _P),
                ("adv", _P), ("ret", _P), ("B", _I32), ("clip", _F), ("value_coef", _F), ("entropy_coef", _F),
                ("grad_loss", _P), ("dlogits", _P), ("dvalues", _P), ("ws", _P), ("cnt", _P), ("stats", _P),
                ("loss", _P)]

class DistillLossArgs(C.Structure):
    """bb_distill_loss_args: grad_loss / dlogits are the backward's, ws / cnt / stats / loss the forward's."""
    _fields_ = [("logits", _P), ("bf16", _I32), ("mask_bits", _P), ("q", _P), ("B", _I32), ("tau", _F),
                ("grad_loss", _P), ("dlogits", _P), ("ws", _P), ("cnt", _P), ("stats", _P), ("loss", _P)]


class GuidedLossArgs(C.Structure):
    """bb_guided_loss_args: q may be NULL iff distill_coef == 0 and coefs_dev is NULL; coefs_dev (device [5] =
    policy, value, entropy, distill, tau) overrides the five scalars; grad_loss / dlogits / dvalues are the
    backward's, ws / cnt / stats / loss the forward's."""
    _fields_ = [("logits", _P), ("values", _P), ("bf16", _I32), ("mask_bits", _P), ("actions", _P), ("old_logp", _P),
                ("adv", _P), ("ret", _P), ("q", _P), ("B", _I32), ("clip", _F), ("policy_coef", _F),
                ("value_coef", _F), ("entropy_coef", _F), ("distill_coef", _F), ("tau", _F), ("coefs_dev", _P),
                ("grad_loss", _P), ("dlogits", _P), ("dvalues", _P), ("ws", _P), ("cnt", _P), ("stats", _P),
                ("loss", _P)]


# name -> (restype, argtypes); exactly the entry points of include/bbvec.h
SIGNATURES = {
    "bb_abi_version": (C.c_int, []),
    "bb_build_id": (C.c_char_p, []),
    "bb_create": (C.c_int, [_I32, _I32, C.POINTER(RewardCfg), _I32, C.POINTER(_P)]),
    "bb_destroy": (None, [_P]),
    "bb_last_error": (C.c_char_p, [_P]),
    "bb_num_envs": (_I32, [_P]),
    "bb_pcg64_seed": (C.c_int, [_U64, C.POINTER(_U64)]),
    "bb_seed": (C.c_int, [_P, _P, _P, _P]),
    "bb_reset": (C.c_int, [_P, _P, _P]),
    "bb_step": (C.c_int, [_P, _P, C.POINTER(StepOut), _P]),
    "bb_rollout": (C.c_int, [_P, _I32, _P, C.POINTER(RolloutOut), _P]),
    "bb_sync": (C.c_int, [_P, _P]),
    "bb_obs": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "bb_device_ptrs": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "bb_snapshot": (C.c_int, [_P, _P, _P, _P, _P]),
    "bb_snapshot_combo": (C.c_int, [_P, _P, _P]),
    "bb_get_state": (C.c_int, [_P, C.POINTER(StateView)]),
    "bb_set_state": (C.c_int, [_P, C.POINTER(StateView)]),
    "bb_debug_counters": (C.c_int, [_P, _P]),
    "bb_random_actions": (C.c_int, [_P, _I32, _U64, _U64, _U64, _P, _P]),
    "bb_afterstates_pos": (C.c_int, [C.POINTER(Positions), _I32, C.POINTER(RewardCfg), C.POINTER(AfterstateOut), _P]),
    "bb_afterstates": (C.c_int, [_P, C.POINTER(AfterstateOut), _P]),
    "bb_greedy_actions_pos": (C.c_int, [C.POINTER(Positions), _I32, C.POINTER(GreedyWeights), _P, _P, _P]),
    "bb_greedy_actions": (C.c_int, [_P, C.POINTER(GreedyWeights), _P, _P, _P]),
    "bb_plan_actions_pos": (C.c_int, [C.POINTER(Positions), _I32, C.POINTER(GreedyWeights), _I32, C.POINTER(PlanOut), _P]),
    "bb_plan_actions": (C.c_int, [_P, C.POINTER(GreedyWeights), _I32, C.POINTER(PlanOut), _P]),
    "bb_greedy_actions_each_pos": (C.c_int, [C.POINTER(Positions), _I32, _P, _P, _P, _P]),
    "bb_greedy_actions_each": (C.c_int, [_P, _P, _P, _P, _P]),
    "bb_plan_actions_each_pos": (C.c_int, [C.POINTER(Positions), _I32, _P, _I32, C.POINTER(PlanOut), _P]),
    "bb_plan_actions_each": (C.c_int, [_P, _P, _I32, C.POINTER(PlanOut), _P]),
    "bb_board_terms_pos": (C.c_int, [_P, _I32, _P, _P]),
    "bb_board_terms": (C.c_int, [_P, _P, _P]),
    "bb_plan_actions_ext_pos": (C.c_int, [C.POINTER(Positions), _I32, _P, C.c_int64, _I32, C.POINTER(PlanOut), _P]),
    "bb_plan_actions_ext": (C.c_int, [_P, _P, C.c_int64, _I32, C.POINTER(PlanOut), _P]),
    "bb_plan_values_pos": (C.c_int, [C.POINTER(Positions), _I32, C.POINTER(GreedyWeights), _I32,
                                     C.POINTER(PlanValuesOut), _P]),
    "bb_plan_values": (C.c_int, [_P, C.POINTER(GreedyWeights), _I32, C.POINTER(PlanValuesOut), _P]),
    "bb_safe_mask_pos": (C.c_int, [C.POINTER(Positions), _I32, _I32, _P, _P]),
    "bb_safe_mask": (C.c_int, [_P, _I32, _P, _P]),
    "bb_refill_census_pos": (C.c_int, [_P, _I32, C.POINTER(CensusOut), _P]),
    "bb_refill_census": (C.c_int, [_P, C.POINTER(CensusOut), _P]),
    "bb_refill_values_pos": (C.c_int, [_P, _P, _P, _I32, C.POINTER(GreedyWeights), _I32, _I32, _U64,
                                       C.POINTER(RefillValuesOut), _P]),
    "bb_refill_values": (C.c_int, [_P, _P, C.POINTER(GreedyWeights), _I32, _I32, _U64, C.POINTER(RefillValuesOut), _P]),
    "bb_plan_values_ext_pos": (C.c_int, [C.POINTER(Positions), _I32, _P, C.c_int64, _I32, C.POINTER(PlanValuesOut),
                                         _P]),
    "bb_plan_values_ext": (C.c_int, [_P, _P, C.c_int64, _I32, C.POINTER(PlanValuesOut), _P]),
    "bb_refill_values_ext_pos": (C.c_int, [_P, _P, _P, _I32, _P, C.c_int64, _I32, _I32, _U64,
                                           C.POINTER(RefillValuesOut), _P]),
    "bb_refill_values_ext": (C.c_int, [_P, _P, _P, C.c_int64, _I32, _I32, _U64, C.POINTER(RefillValuesOut), _P]),
    "bb_play_plan_pos": (C.c_int, [C.POINTER(Positions), _I32, _P, C.POINTER(PlayPlanOut), _P]),
    "bb_plan2_work_bytes": (C.c_int64, [_I32, _I32, _I32]),
    "bb_plan2_values_pos": (C.c_int, [C.POINTER(Positions), _P, _I32, _P, C.c_int64, _I32, _I32, _I32, _U64, _P,
                                      C.c_int64, C.POINTER(Plan2Out), _P]),
    "bb_plan2_values": (C.c_int, [_P, _P, _P, C.c_int64, _I32, _I32, _I32, _U64, _P, C.c_int64,
                                  C.POINTER(Plan2Out), _P]),
    "bb_playout_values_pos": (C.c_int, [_P, _P, _P, _I32, _P, C.c_int64, _I32, _I32, _I32, _U64,
                                        C.POINTER(PlayoutOut), _P]),
    "bb_playout_values": (C.c_int, [_P, _P, _P, C.c_int64, _I32, _I32, _I32, _U64, C.POINTER(PlayoutOut), _P]),
    "bb_masked_sample": (C.c_int, [_P, _P, _I32, _P, _U64, _U64, _U64, _I32, _P, _P, _P, _P, _P]),
    "bb_masked_sample_dstep": (C.c_int, [_P, _P, _I32, _U64, _P, _U64, _U64, _I32, _P, _P, _P, _P]),
    "bb_gae": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _F, _F, _P, _P, _P]),
    "bb_gather_obs": (C.c_int, [_P, _P, _P, _P, _I32, _P, _P, _P]),
    "bb_bn_workspace_bytes": (C.c_int64, [_I32, _I32, _I32, _I32, _I32]),
    "bb_bn_forward": (C.c_int, [C.POINTER(BnFwd), _P]),
    "bb_bn_backward": (C.c_int, [C.POINTER(BnBwd), _P]),
    "bb_conv3x3_workspace_bytes": (C.c_int64, [_I32, _I32, _I32]),
    "bb_conv3x3_prep": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _P]),
    "bb_conv3x3_prep_multi": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P]),
    "bb_conv3x3_forward": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "bb_conv3x3_forward_add": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "bb_conv3x3_stats_blocks": (C.c_int32, [_I32, _I32]),
    "bb_conv3x3_forward_stats": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "bb_conv3x3_forward_bstats": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _I32, _P, _P]),
    "bb_conv3x3_wgrad": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "bb_conv3x3_wgrad_chunks": (C.c_int32, [_I32, _I32, _I32]),
    "bb_conv3x3_wgrad_partial": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "bb_conv3x3_wgrad_reduce": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P]),
    "bb_conv3x3_f32_prep": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _P]),
    "bb_conv3x3_f32_forward": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "bb_linear_f32": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "bb_ppo_loss_workspace_bytes": (C.c_int64, [_I32]),
    "bb_ppo_loss_forward": (C.c_int, [C.POINTER(PpoLossArgs), _P]),
    "bb_ppo_loss_backward": (C.c_int, [C.POINTER(PpoLossArgs), _P]),
    "bb_ppo_loss_fused": (C.c_int, [C.POINTER(PpoLossArgs), _P]),
    "bb_distill_loss_workspace_bytes": (C.c_int64, [_I32]),
    "bb_distill_loss_forward": (C.c_int, [C.POINTER(DistillLossArgs), _P]),
    "bb_distill_loss_backward": (C.c_int, [C.POINTER(DistillLossArgs), _P]),
    "bb_distill_loss_fused": (C.c_int, [C.POINTER(DistillLossArgs), _P]),
    "bb_guided_loss_workspace_bytes": (C.c_int64, [_I32]),
    "bb_guided_loss_forward": (C.c_int, [C.POINTER(GuidedLossArgs), _P]),
    "bb_guided_loss_backward": (C.c_int, [C.POINTER(GuidedLossArgs), _P]),
    "bb_guided_loss_fused": (C.c_int, [C.POINTER(GuidedLossArgs), _P]),
    "bb_adam_clip_workspace_bytes": (C.c_int64, [_I32, _P]),
    "bb_adam_clip_step": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double, _F,
                                    _P, _P, _P]),
    "bb_cast_multi": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _P, _P]),
    "bb_dropout_forward": (C.c_int, [_P, C.c_int64, _F, _P, _P]),
    "bb_conv_in_wgrad_workspace_bytes": (C.c_int64, [_I32]),
    "bb_conv_in_forward": (C.c_int, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "bb_conv_in_wgrad": (C.c_int, [_P, _I32, _P, _I32, _P, _I32, _P, _P]),
    "bb_conv_in_forward_prep": (C.c_int, [_P, _I32, _P, _I32, _I32, _P, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "bb_linear_n1_workspace_bytes": (C.c_int64, [_I32, _I32]),
    "bb_linear_n1_counters": (C.c_int32, [_I32]),
    "bb_linear_n1_forward": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "bb_linear_n1_backward": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "bb_linear_wgrad_workspace_bytes": (C.c_int64, [_I32, _I32, _I32]),
    "bb_linear_wgrad_counters": (C.c_int32, [_I32, _I32]),
    "bb_linear_wgrad": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    "bb_linear_bgrad_workspace_bytes": (C.c_int64, [_I32, _I32]),
    "bb_linear_bgrad_counters": (C.c_int32, [_I32]),
    "bb_linear_bgrad": (C.c_int, [_P, _P, _I32, _I32, _F, _P, _P, _P, _P, _P]),
    "bb_linear_bgrad2": (C.c_int, [_P, _P, _I32, _P, _I32, _I32, _F, _P, _P, _P, _P, _P]),
}

# the env entry points, which the host backend (libbbvec_host.so) exports too
HOST_SYMBOLS = ("bb_abi_version", "bb_build_id", "bb_create", "bb_destroy", "bb_last_error", "bb_num_envs", "bb_pcg64_seed",
                "bb_seed", "bb_reset", "bb_step", "bb_rollout", "bb_sync", "bb_obs", "bb_device_ptrs", "bb_snapshot",
                "bb_snapshot_combo", "bb_get_state", "bb_set_state", "bb_random_actions", "bb_afterstates_pos",
                "bb_afterstates",
                "bb_greedy_actions_pos", "bb_greedy_actions", "bb_plan_actions_pos", "bb_plan_actions",
                "bb_greedy_actions_each_pos", "bb_greedy_actions_each", "bb_plan_actions_each_pos",
                "bb_plan_actions_each",
                "bb_board_terms_pos", "bb_board_terms", "bb_plan_actions_ext_pos", "bb_plan_actions_ext",
                "bb_plan_values_pos", "bb_plan_values", "bb_safe_mask_pos", "bb_safe_mask",
                "bb_refill_census_pos", "bb_refill_census", "bb_refill_values_pos", "bb_refill_values",
                "bb_plan_values_ext_pos", "bb_plan_values_ext", "bb_refill_values_ext_pos", "bb_refill_values_ext",
                "bb_play_plan_pos", "bb_plan2_work_bytes", "bb_plan2_values_pos", "bb_plan2_values",
                "bb_playout_values_pos", "bb_playout_values")

_lib = None
_host = None
_lock = threading.Lock()


def load(path: str | None = None):
    """Load libbbvec.so (once) and bind every symbol of bbvec.h."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise BBNativeError(
                f"HIP library not found at {p}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)"
            )
        lib = C.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError == missing export
            fn.restype = res
            fn.argtypes = args
        v = lib.bb_abi_version()
        if v != ABI_VERSION:
            raise BBNativeError(f"libbbvec ABI version mismatch ({v}, expected {ABI_VERSION})")
        if path is None and "BBVEC_LIB" not in os.environ:
            _check_build_id(lib, p, host=False)
        if path is None:
            _lib = lib
        return lib


def _check_build_id(lib, p: str, host: bool) -> None:
    """Refuse a library that was not built from the sources beside it (bb_build_id against
    runtime/build.py's hash of csrc/, include/bbvec.h and the flags).  Explicit variant builds
    (load(path), BBVEC_LIB) are diagnostics and skip the check."""
    from . import build as B

    want = B.host_source_id() if host else B.source_id()
    have = lib.bb_build_id().decode()
    if have != want:
        raise BBNativeError(
            f"{os.path.basename(p)} was built from other sources (build id {have}, these sources {want}); "
            "rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")


def build_id(host: bool = False) -> str:
    """The loaded library's build id (bb_build_id)."""
    return (load_host() if host else load()).bb_build_id().decode()


def load_host():
    """Load libbbvec_host.so (once), the host backend of the env entry points."""
    global _host
    with _lock:
        if _host is not None:
            return _host
        if not os.path.exists(HOST_LIB_PATH):
            raise BBNativeError(f"host backend not found at {HOST_LIB_PATH}; build it with "
                                "`python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(HOST_LIB_PATH)
        for name in HOST_SYMBOLS:
            res, args = SIGNATURES[name]
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.bb_abi_version() != ABI_VERSION:
            raise BBNativeError("libbbvec_host ABI version mismatch")
        _check_build_id(lib, HOST_LIB_PATH, host=True)
        _host = lib
        return lib


def last_error(handle=None, lib=None) -> str:
    msg = (lib or load()).bb_last_error(handle)
    return msg.decode() if msg else ""


def check(rc: int, what: str, handle=None, lib=None) -> None:
    if rc != BB_OK:
        raise BBNativeError(f"{what} failed ({rc}): {last_error(handle, lib)}")


def pcg64_seed(seed: int):
    """numpy-exact default_rng(seed) PCG64 words {state_hi, state_lo, inc_hi, inc_lo}."""
    out = (_U64 * 4)()
    check(load().bb_pcg64_seed(seed, out), "bb_pcg64_seed")
    return [int(x) for x in out]


def reward_cfg(rewards: dict) -> RewardCfg:
    cfg = RewardCfg()
    for name, _ in RewardCfg._fields_:
        setattr(cfg, name, float(rewards[name]))
    return cfg
