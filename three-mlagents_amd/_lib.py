"""ctypes binding of csrc/libtma_hip.so (the C ABI declared in include/tma.h).

The HIP library is the product: there is no CPU or PyTorch fallback.  If the shared object is missing this
module raises ImportError telling the user to build it (`python -c "import __graft_entry__ as g; g.build()"`).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("TMA_LIB_PATH") or os.path.join(_HERE, "csrc", "libtma_hip.so")  # (TMA_LIB_PATH: diagnostic builds of the same ABI)

TMA_OK, TMA_ERR_INVALID, TMA_ERR_UNKNOWN_TASK, TMA_ERR_HIP = 0, 1, 2, 3
ACT_I32, ACT_I64, ACT_F32 = 0, 1, 2
EP_STRIDE = 1 << 20
EV_SCRATCH_DOUBLES = 1536  # include/tma.h TMA_EV_SCRATCH_DOUBLES
VECNORM_ONE_LAUNCH_MAX = 256  # include/tma.h TMA_VECNORM_ONE_LAUNCH_MAX
GATHER_BLOCKS = 2048  # csrc/tma_workspace.h GATHER_BLOCKS: tma_rollout_gather's grid cap (workgroups of four waves); the tests size a case past it
ROLLOUT_NORM_PER_STEP, ROLLOUT_NORM_FUSED_DISC_F32, ROLLOUT_NORM_FUSED_CONT_F32 = 0, 1, 2  # include/tma.h TMA_ROLLOUT_NORM_*: tma_rollout_norm_plan
# include/tma.h TMA_ROLLOUT_FAMILY_* / TMA_ROLLOUT_PLAN_NORM_*: tma_debug_plan_rollout, tma_debug_last_rollout_plan
ROLLOUT_FAMILIES = ("PER_STEP", "H64", "BF16_DISC", "BF16_BOX_TWO_NET", "BF16_BOX_PI", "F32_DISC", "F32_BOX")
ROLLOUT_PLAN_NORM_NONE, ROLLOUT_PLAN_NORM_TRAINING, ROLLOUT_PLAN_NORM_FROZEN = 0, 1, 2

_vp, _i32, _i64, _u32, _f64 =C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_double



class PolicyDims(C.Structure):
    _fields_ = [("obs_dim", _i32), ("hidden", _i32), ("act_dim", _i32), ("continuous", _i32), ("mfma_dtype", _i32), ("device", _i32), ("activation", _i32)]


class Rollout(C.Structure):
    _fields_ = [("obs", _vp), ("actions", _vp), ("log_probs", _vp), ("advantages", _vp), ("returns", _vp), ("T", _i32), ("N", _i64),
                ("packed", _vp)]  # (optional sample records, tma_ppo_pack_samples; None = absent)


class Minibatch(C.Structure):
    _fields_ = [("indices", _vp), ("perm_seed", _u32), ("perm_epoch", _u32), ("start", _i64), ("count", _i64), ("prepared_batch", _i64), ("stats_count", _i64)]


class PPOHParams(C.Structure):
    _fields_ = [("clip_range", _f64), ("ent_coef", _f64), ("vf_coef", _f64), ("normalize_advantage", _i32)]


class A2CHParams(C.Structure):
    _fields_ = [("ent_coef", _f64), ("vf_coef", _f64), ("normalize_advantage", _i32)]


class RolloutBuffers(C.Structure):
    _fields_ = [("obs", _vp), ("actions", _vp), ("rewards", _vp), ("values", _vp), ("log_probs", _vp), ("terminated", _vp),
                ("truncated", _vp), ("terminal_obs", _vp), ("last_values", _vp), ("N", _i64), ("terminal_obs_slots", _i32)]


class Replay(C.Structure):  # include/tma.h tma_replay: the planes of a replay buffer and their geometry
    _fields_ = [("obs", _vp), ("next_obs", _vp), ("actions", _vp), ("rewards", _vp), ("terminated", _vp), ("truncated", _vp), ("capacity", _i32),
                ("n_envs", _i64), ("obs_dim", _i32), ("act_dim", _i32), ("continuous", _i32)]


class DQNHParams(C.Structure):  # include/tma.h tma_dqn_hparams
    _fields_ = [("total_timesteps", _i64), ("learning_starts", _i64), ("batch_size", _i64), ("target_update_interval", _i64), ("train_freq", _i32),
                ("gradient_steps", _i32), ("n_step", _i32), ("tau", _f64), ("gamma", _f64), ("exploration_fraction", _f64),
                ("exploration_initial_eps", _f64), ("exploration_final_eps", _f64), ("learning_rate", _f64), ("max_grad_norm", _f64),
                ("rng_seed", _u32), ("sample_seed", _u32), ("env_offset", _u32)]


class DQNBuffers(C.Structure):  # include/tma.h tma_dqn_buffers
    _fields_ = [("last_obs", _vp), ("actions", _vp), ("step_obs", _vp), ("rewards", _vp), ("term", _vp), ("trunc", _vp), ("term_obs", _vp),
                ("s_obs", _vp), ("s_actions", _vp), ("s_next_obs", _vp), ("s_dones", _vp), ("s_rewards", _vp), ("s_discounts", _vp),
                ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("stats", _vp), ("td_workspace", _vp), ("td_workspace_bytes", _i64),
                ("opt_workspace", _vp)]


class DQNCounters(C.Structure):  # include/tma.h tma_dqn_counters
    _fields_ = [("num_timesteps", _i64), ("n_calls", _i64), ("pos", _i64), ("full", _i32), ("draw", _u32), ("collect_step", _u32),
                ("adam_step", _i64), ("n_updates", _i64)]


SAC_SAMPLE, SAC_DETERMINISTIC, SAC_UNIFORM = 0, 1, 2  # include/tma.h TMA_SAC_*: tma_sac_act's mode
SAC_GRID_CAP = 64  # csrc/tma_sac.hip SAC_GRID_CAP: workgroups of a gradient kernel at the most; the tests size a case past it


class SACDims(C.Structure):  # include/tma.h tma_sac_dims
    _fields_ = [("obs_dim", _i32), ("act_dim", _i32), ("hidden", _i32), ("activation", _i32), ("device", _i32)]


class SACOffsets(C.Structure):  # include/tma.h tma_sac_offsets
    _fields_ = [(k, _i32) for k in ("a_W1", "a_b1", "a_W2", "a_b2", "a_Wmu", "a_bmu", "a_Wls", "a_bls", "n_actor",
                                    "q_W1", "q_b1", "q_W2", "q_b2", "q_W3", "q_b3", "n_q", "n_critic")]


class SACHParams(C.Structure):  # include/tma.h tma_sac_hparams
    _fields_ = [("learning_starts", _i64), ("batch_size", _i64), ("target_update_interval", _i64), ("train_freq", _i32), ("gradient_steps", _i32),
                ("n_step", _i32), ("auto_ent_coef", _i32), ("tau", _f64), ("gamma", _f64), ("learning_rate", _f64), ("target_entropy", _f64),
                ("rng_seed", _u32), ("sample_seed", _u32), ("env_offset", _u32)]


class SACBuffers(C.Structure):  # include/tma.h tma_sac_buffers
    _fields_ = [(k, _vp) for k in ("last_obs", "actions", "step_obs", "rewards", "term", "trunc", "term_obs", "s_obs", "s_actions", "s_next_obs", "s_dones",
                                   "s_rewards", "s_discounts", "actor_grad", "actor_exp_avg", "actor_exp_avg_sq", "critic_grad", "critic_exp_avg",
                                   "critic_exp_avg_sq", "ent_grad", "ent_exp_avg", "ent_exp_avg_sq", "critic_stats", "actor_stats", "workspace")] + [
                                       ("workspace_bytes", _i64)]


class SACCounters(C.Structure):  # include/tma.h tma_sac_counters
    _fields_ = [("num_timesteps", _i64), ("n_calls", _i64), ("pos", _i64), ("full", _i32), ("draw", _u32), ("collect_step", _u32),
                ("adam_step", _i64), ("n_updates", _i64)]


TD3_DETERMINISTIC, TD3_NOISY, TD3_UNIFORM = 0, 1, 2  # include/tma.h TMA_TD3_*: tma_td3_act's mode


class TD3Offsets(C.Structure):  # include/tma.h tma_td3_offsets
    _fields_ = [(k, _i32) for k in ("a_W1", "a_b1", "a_W2", "a_b2", "a_Wmu", "a_bmu", "n_actor", "q_W1", "q_b1", "q_W2", "q_b2", "q_W3", "q_b3", "n_q", "n_critic")]


class TD3Noise(C.Structure):  # include/tma.h tma_td3_noise
    _fields_ = [("mean", C.c_float * 8), ("sigma", C.c_float * 8)]


class TD3HParams(C.Structure):  # include/tma.h tma_td3_hparams
    _fields_ = [("learning_starts", _i64), ("batch_size", _i64), ("policy_delay", _i64), ("train_freq", _i32), ("gradient_steps", _i32), ("n_step", _i32),
                ("use_action_noise", _i32), ("tau", _f64), ("gamma", _f64), ("learning_rate", _f64), ("target_policy_noise", _f64),
                ("target_noise_clip", _f64), ("action_noise", TD3Noise), ("rng_seed", _u32), ("sample_seed", _u32), ("env_offset", _u32)]


class TD3Buffers(C.Structure):  # include/tma.h tma_td3_buffers
    _fields_ = [(k, _vp) for k in ("last_obs", "actions", "step_obs", "rewards", "term", "trunc", "term_obs", "s_obs", "s_actions", "s_next_obs", "s_dones",
                                   "s_rewards", "s_discounts", "actor_grad", "actor_exp_avg", "actor_exp_avg_sq", "critic_grad", "critic_exp_avg",
                                   "critic_exp_avg_sq", "critic_stats", "actor_stats", "workspace")] + [("workspace_bytes", _i64)]


class TD3Counters(C.Structure):  # include/tma.h tma_td3_counters
    _fields_ = [("num_timesteps", _i64), ("n_calls", _i64), ("pos", _i64), ("full", _i32), ("draw", _u32), ("collect_step", _u32),
                ("critic_adam_step", _i64), ("actor_adam_step", _i64), ("n_updates", _i64)]


_pd = C.POINTER(PolicyDims)
_sd = C.POINTER(SACDims)

# name -> (restype, argtypes); every symbol include/tma.h declares
SIGNATURES = {
    "tma_version": (_i32, []),
    "tma_last_error": (C.c_char_p, []),
    "tma_task_id": (_i32, [C.c_char_p, C.POINTER(_i32)]),
    "tma_task_obs_dim": (_i32, [_i32]),
    "tma_task_num_actions": (_i32, [_i32]),
    "tma_task_act_dim": (_i32, [_i32]),
    "tma_task_state_dim": (_i32, [_i32]),
    "tma_task_max_episode_steps": (_i32, [_i32]),
    "tma_env_create": (_i32, [_i32, _i64, _i32, _u32, _u32, _i32, C.POINTER(_vp)]),
    "tma_env_destroy": (_i32, [_vp]),
    "tma_env_seed": (_i32, [_vp, _u32]),
    "tma_env_set_reward64": (_i32, [_vp, _vp, _i64]),
    "tma_env_reset": (_i32, [_vp, _vp, _vp]),
    "tma_env_step": (_i32, [_vp, _vp, _i32, _u32, _u32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tma_env_step_repeat": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tma_env_steps_until_refill": (_i32, [_vp, C.POINTER(_i32)]),
    "tma_env_refill": (_i32, [_vp, _vp]),
    "tma_env_set_option": (_i32, [_vp, C.c_char_p, _i64]),
    "tma_env_get_state": (_i32, [_vp, _vp, _vp]),
    "tma_env_set_state": (_i32, [_vp, _vp, _vp]),
    "tma_env_episode_index": (_i32, [_vp, _vp, _vp]),
    "tma_env_episode_log": (_i32, [_vp, _i64]),
    "tma_monitor_append_rows": (_i32, [C.c_char_p, _vp, _vp, _vp, _i64]),
    "tma_env_pop_episode_log": (_i32, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "tma_env_pop_episode_stats": (_i32, [_vp, C.POINTER(_f64), _vp]),
    "tma_env_clear_episode_log": (_i32, [_vp, _vp]),
    "tma_env_detach_episode_log": (_i32, [_vp]),
    "tma_env_pop_detached_episode_log": (_i32, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_f64), _vp]),
    "tma_gae": (_i32, [_vp, _vp, _vp, _vp, _vp, _f64, _f64, _i32, _i64, _vp, _vp, _vp]),
    "tma_gae_flags": (_i32, [_vp, _vp, _vp, _vp, _vp, _f64, _f64, _i32, _i64, _vp, _vp, _vp]),
    "tma_explained_variance": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "tma_policy_param_count": (_i32, [_pd, C.POINTER(_i64), C.POINTER(_i64)]),
    "tma_policy_param_offsets": (_i32, [_pd, C.POINTER(_i32)]),
    "tma_policy_sync": (_i32, [_vp, _pd, _vp]),
    "tma_policy_act": (_i32, [_vp, _pd, _vp, _i64, _u32, _u32, _u32, _i32, _vp, _vp, _vp, _vp]),
    "tma_policy_act_bootstrap": (_i32, [_vp, _pd, _vp, _i64, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _f64, _vp, _vp]),
    "tma_policy_evaluate_actions": (_i32, [_vp, _pd, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "tma_policy_vjp_workspace_bytes": (_i64, [_pd, _i64]),
    "tma_policy_evaluate_actions_backward": (_i32, [_vp, _pd, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_policy_head": (_i32, [_vp, _pd, _vp, _i64, _vp, _vp, _vp]),
    "tma_policy_head_backward": (_i32, [_vp, _pd, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_policy_evaluate_actions_vjp": (_i32, [_vp, _pd, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_policy_head_vjp": (_i32, [_vp, _pd, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_policy_values": (_i32, [_vp, _pd, _vp, _i64, _vp, _vp]),
    "tma_policy_bootstrap": (_i32, [_vp, _pd, _vp, _vp, _i64, _f64, _vp, _vp]),
    "tma_ppo_workspace_bytes": (_i64, [_pd]),
    "tma_ppo_packed_floats": (_i64, [_pd, _i32, _i64]),
    "tma_ppo_pack_samples": (_i32, [C.POINTER(Rollout), _pd, _vp, _vp]),
    "tma_ppo_minibatch_grad": (_i32, [_vp, _pd, C.POINTER(Rollout), C.POINTER(Minibatch), C.POINTER(PPOHParams), _vp, _vp, _vp]),
    "tma_debug_time_grad_kernel": (_i32, [_i32]),
    "tma_debug_poison_lds": (_i32, [_u32, _vp]),
    "tma_debug_last_grad_kernel_us": (_i32, [C.POINTER(C.c_float)]),
    "tma_debug_last_dispatch": (_i32, [C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "tma_debug_plan_dispatch": (_i32, [_pd, _i32, _i64, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32)]),
    "tma_debug_last_rollout_waves": (_i32, []),
    "tma_debug_last_prep_fold": (_i32, [C.POINTER(_i32), C.POINTER(_i32)]),
    "tma_ppo_epoch_prepare": (_i32, [C.POINTER(Rollout), C.POINTER(Minibatch), _i64, _pd, _vp, _vp]),
    "tma_ppo_epoch_adv_sums": (_i32, [_vp, _pd, _i64, _i64, _vp, _i32, _vp]),
    "tma_ppo_adam_step": (_i32, [_vp, _vp, _vp, _vp, _pd, _i64, _f64, _f64, _f64, _f64, _f64, _f64, _vp, _vp]),
    "tma_ppo_adam_step_local": (_i32, [_vp, _vp, _vp, _vp, _pd, _i64, _f64, _f64, _f64, _f64, _f64, _vp, _vp, _i64]),
    "tma_ppo_permutation": (_i32, [_u32, _u32, _i64, _vp]),
    "tma_rollout_gather": (_i32, [C.POINTER(Rollout), _vp, _pd, C.POINTER(Minibatch), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tma_replay_add": (_i32, [C.POINTER(Replay), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tma_replay_sample": (_i32, [C.POINTER(Replay), _i32, _i32, _i32, _f64, _u32, _u32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tma_egreedy_actions": (_i32, [_vp, _i64, _i32, _f64, _u32, _u32, _u32, _vp, _vp]),
    "tma_dqn_act": (_i32, [_vp, _pd, _vp, _i64, _f64, _u32, _u32, _u32, _vp, _vp, _vp]),
    "tma_dqn_workspace_bytes": (_i64, [_pd, _i64]),
    "tma_dqn_td_grad": (_i32, [_vp, _vp, _pd, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_dqn_target_update": (_i32, [_vp, _vp, _pd, _f64, _vp]),
    "tma_dqn_epsilon": (_f64, [C.POINTER(DQNHParams), _i64]),
    "tma_dqn_iterations_local": (_i32, [_vp, _vp, _vp, _pd, C.POINTER(Replay), C.POINTER(DQNBuffers), C.POINTER(DQNHParams), C.POINTER(DQNCounters),
                                        _i32, _vp]),
    "tma_sac_param_offsets": (_i32, [_sd, C.POINTER(SACOffsets)]),
    "tma_sac_act": (_i32, [_vp, _sd, _vp, _i64, _i32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tma_sac_workspace_bytes": (_i64, [_sd, _i64]),
    "tma_sac_critic_grad": (_i32, [_vp, _vp, _vp, _vp, _sd, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_sac_actor_grad": (_i32, [_vp, _vp, _vp, _sd, _vp, _i64, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_sac_ent_coef_grad": (_i32, [_vp, _f64, _vp, _vp]),
    "tma_adam_step_flat": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _f64, _f64, _f64, _f64, _vp]),
    "tma_polyak_update": (_i32, [_vp, _vp, _i64, _f64, _vp]),
    "tma_sac_iterations_local": (_i32, [_vp, _vp, _vp, _vp, _vp, _sd, C.POINTER(Replay), C.POINTER(SACBuffers), C.POINTER(SACHParams), C.POINTER(SACCounters),
                                        _i32, _vp]),
    "tma_td3_param_offsets": (_i32, [_sd, C.POINTER(TD3Offsets)]),
    "tma_td3_act": (_i32, [_vp, _sd, _vp, _i64, _i32, C.POINTER(TD3Noise), _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "tma_td3_workspace_bytes": (_i64, [_sd, _i64]),
    "tma_td3_critic_grad": (_i32, [_vp, _vp, _vp, _sd, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _f64, _f64, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_td3_actor_grad": (_i32, [_vp, _vp, _sd, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tma_td3_iterations_local": (_i32, [_vp, _vp, _vp, _vp, _vp, _sd, C.POINTER(Replay), C.POINTER(TD3Buffers), C.POINTER(TD3HParams), C.POINTER(TD3Counters),
                                        _i32, _vp]),
    "tma_ppo_persist_fallbacks": (_i32, [_vp, C.POINTER(_i64), _vp]),
    "tma_ppo_train_epoch_local": (_i32, [_vp, _pd, C.POINTER(Rollout), _u32, _u32, _i64, C.POINTER(PPOHParams), _vp, _vp, _vp, _i64, _f64, _f64, _f64, _f64,
                                         _f64, _vp, _vp]),
    "tma_ppo_train_epochs_local": (_i32, [_vp, _pd, C.POINTER(Rollout), _u32, _u32, _i32, _i64, C.POINTER(PPOHParams), _vp, _vp, _vp, _i64, _f64, _f64, _f64, _f64,
                                          _f64, _vp, _vp]),
    "tma_ppo_train_epoch_dp": (_i32, [_vp, _pd, C.POINTER(Rollout), _u32, _u32, _i64, _i64, _i32, C.POINTER(PPOHParams), _vp, _vp, _vp, _i64, _f64, _f64, _f64,
                                      _f64, _f64, _f64, None, _vp, _vp, _vp]),  # (None: the AllReduceFn slot, filled in below)
    "tma_ppo_pop_stats": (_i32, [_vp, C.POINTER(_f64), _vp]),
    "tma_ppo_stats_staging_bytes": (_i64, []),
    "tma_ppo_stats_enqueue": (_i32, [_vp, _vp, _vp]),
    "tma_ppo_stats_fold": (_i32, [_vp, C.POINTER(_f64)]),
    "tma_comm_available": (_i32, []),
    "tma_comm_unique_id": (_i32, [_vp]),
    "tma_comm_create": (_i32, [_vp, _i32, _i32, _i32, C.POINTER(_vp)]),
    "tma_comm_destroy": (_i32, [_vp]),
    "tma_comm_bind_stream": (_i32, [_vp, _vp]),
    "tma_comm_allreduce": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "tma_comm_allreduce_cb": (_i32, [_vp, _vp, _i64]),
    "tma_comm_timing": (_i32, [_vp, _i32]),
    "tma_comm_pop_timing": (_i32, [_vp, _vp, _i32, C.POINTER(_i32), C.POINTER(_i64)]),
    "tma_comm_create_p2p": (_i32, [_i32, _i32, _i32, C.POINTER(_vp)]),
    "tma_comm_p2p_prepare": (_i32, [_vp, _i64, _vp]),
    "tma_comm_p2p_attach": (_i32, [_vp, _vp]),
    "tma_comm_p2p_attach_local": (_i32, [_vp, _vp]),
    "tma_comm_p2p_enable": (_i32, [_vp, _i32]),
    "tma_comm_p2p_set_timeout": (_i32, [_vp, C.c_double]),
    "tma_comm_p2p_status": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i64)]),
    "tma_ppo_stats_clear": (_i32, [_vp, _vp]),
    "tma_rmsprop_step": (_i32, [_vp, _vp, _vp, _pd, _f64, _f64, _f64, _f64, _f64, _vp, _vp]),
    "tma_rmsprop_step_local": (_i32, [_vp, _vp, _vp, _pd, _f64, _f64, _f64, _f64, _vp, _vp, _i64]),
    "tma_a2c_update_local": (_i32, [_vp, _pd, C.POINTER(Rollout), C.POINTER(A2CHParams), _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp]),
    "tma_a2c_grad": (_i32, [_vp, _pd, C.POINTER(Rollout), C.POINTER(A2CHParams), _vp, _vp, _vp]),
    "tma_a2c_iterations_local": (_i32, [_vp, _vp, _pd, C.POINTER(RolloutBuffers), _vp, _vp, _vp, _i32, _u32, _u32, _u32, _f64, _f64, _i32, _i32,
                                        C.POINTER(A2CHParams), _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp]),
    "tma_a2c_stats_fold": (_i32, [_vp, C.POINTER(_f64)]),
    "tma_rollout_collect": (_i32, [_vp, _vp, _pd, C.POINTER(RolloutBuffers), _i32, _i32, _i32, _u32, _u32, _u32, _f64, _i32, _i32, _vp]),
    "tma_vecnorm_create": (_i32, [_i32, _i64, _i32, _i32, _f64, _f64, _f64, _f64, _i32, C.POINTER(_vp)]),
    "tma_vecnorm_destroy": (_i32, [_vp]),
    "tma_vecnorm_set_flags": (_i32, [_vp, _i32, _i32]),
    "tma_vecnorm_reset": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "tma_vecnorm_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tma_vecnorm_normalize_obs": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "tma_vecnorm_unnormalize_obs": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "tma_vecnorm_normalize_reward": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "tma_vecnorm_unnormalize_reward": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "tma_vecnorm_get_stats": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "tma_vecnorm_set_stats": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "tma_vecnorm_copy_stats": (_i32, [_vp, _vp, _vp]),
    "tma_vecnorm_get_returns": (_i32, [_vp, _vp, _vp]),
    "tma_vecnorm_get_original": (_i32, [_vp, _vp, _vp, _vp]),
    "tma_rollout_collect_norm": (_i32, [_vp, _vp, _vp, _pd, C.POINTER(RolloutBuffers), _i32, _i32, _i32, _u32, _u32, _u32, _f64, _i32, _i32, _i32, _vp]),
    "tma_rollout_norm_plan": (_i32, [_i32, _pd, _i64, _i32]),
    "tma_debug_last_rollout_norm_path": (_i32, []),
    "tma_debug_plan_rollout": (_i32, [_i32, _pd, _i64, _i32, _i32, _i32, C.POINTER(_i32)]),
    "tma_debug_last_rollout_plan": (_i32, [C.POINTER(_i32)]),
}

# tma_allreduce_fn (include/tma.h): int (*)(void *ctx, float *buffer, int64_t count)
AllReduceFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
SIGNATURES["tma_ppo_train_epoch_dp"] = (_i32, [AllReduceFn if a is None else a for a in SIGNATURES["tma_ppo_train_epoch_dp"][1]])

_lib = None


def lib():
    """Load libtma_hip.so once; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} is missing: the HIP extension is the only compute path of three-mlagents_amd. "
                "Build it with `make -C three-mlagents_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`)."
            )
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def last_error() -> str:
    msg = lib().tma_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status: int) -> None:
    """Map a TMA_* status to the exception type the reference raises for the same condition."""
    if status == TMA_OK:
        return
    msg = last_error()
    if status == TMA_ERR_UNKNOWN_TASK:
        raise KeyError(msg)  # registry.get_task: backend/mlagents/registry.py:359-362
    if status == TMA_ERR_INVALID:
        raise ValueError(msg)  # registry.make_env / train_task: registry.py:368-369, training.py:105-114
    raise RuntimeError(msg)  # HIP / RCCL failures


def task_id(name: str) -> int:
    out = _i32(0)
    check(lib().tma_task_id(name.encode(), C.byref(out)))
    return out.value


def ptr(t):
    """Device (or host) pointer of a torch tensor / numpy array, or None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return t.ctypes.data_as(C.c_void_p)


def stream_ptr(device=None):
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
