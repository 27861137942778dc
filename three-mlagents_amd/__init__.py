"""three-mlagents_amd: MI355X-native vectorized-env + PPO engine for the three-mlagents Gymnasium tasks.

The compute is libtma_hip.so (C ABI: include/tma.h).  Host side: `vec_env` (SB3 VecEnv / Gymnasium VectorEnv surfaces), `envs`
(single Gymnasium-shaped env), `ppo` (SB3-shaped PPO), `harness` (make_vector_env / train_task / evaluate_model), `tasks`
(the engine's task table).  Import as `three_mlagents_amd` (alias package at the repo root; the directory name has a hyphen).
"""
__version__ = "0.2.0"

from .tasks import ENGINE_TASKS, EngineTask, make_env, resolve  # noqa: E402

__all__ = ["ENGINE_TASKS", "EngineTask", "make_env", "resolve", "__version__", "PPO", "A2C", "DQN", "SAC", "TD3", "NormalActionNoise", "RolloutBuffer", "RolloutBufferSamples", "ReplayBuffer",
           "ReplayBufferSamples"]


def __getattr__(name):  # the algorithm classes import torch: on first use, not with the task table
    if name == "PPO":
        from .ppo import PPO

        return PPO
    if name == "A2C":
        from .a2c import A2C

        return A2C
    if name == "DQN":
        from .dqn import DQN

        return DQN
    if name == "SAC":
        from .sac import SAC

        return SAC
    if name == "TD3":
        from .td3 import TD3

        return TD3
    if name == "NormalActionNoise":
        from .td3 import NormalActionNoise

        return NormalActionNoise
    if name in ("RolloutBuffer", "RolloutBufferSamples"):
        from . import rollout_buffer

        return getattr(rollout_buffer, name)
    if name in ("ReplayBuffer", "ReplayBufferSamples"):
        from . import replay_buffer

        return getattr(replay_buffer, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
