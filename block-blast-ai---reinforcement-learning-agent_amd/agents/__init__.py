"""Masked-PPO agent (rollout kernels on HIP, update in PyTorch-ROCm + RCCL)."""
from .base import BaseAgent  # noqa: F401
from .greedy import (DEFAULT_WEIGHTS, GreedyAgent, HandPlanAgent, PopulationPlanAgent,  # noqa: F401
                     PlayoutPlanAgent, PopulationTwoHandAgent, RandomAgent)
from .ppo import PackedRolloutBuffer, PPOAgent, PPOConfig, RolloutBuffer, broadcast_parameters  # noqa: F401
