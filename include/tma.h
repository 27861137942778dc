/*
 * tma.h -- C ABI of libtma_hip.so: the MI355X (gfx950) vector-env + PPO hot path for
 * lukehollis/three-mlagents.  Plain pointers and sizes only; every device pointer is HBM on the
 * handle's device; `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *
 * The reference has no FFI: its boundary is a Python API.  Each entry point cites
 * the reference interface (path:line under /root/reference/) whose work it replaces.  The Python
 * shim (three-mlagents_amd/_lib.py) binds these with ctypes and mirrors the reference's operator
 * names; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Every function returns a TMA_* status; tma_last_error() gives the message (thread-local).
 * Status -> Python exception in the shim:  INVALID -> ValueError (registry.py:368-369,
 * training.py:105-114), UNKNOWN_TASK -> KeyError (registry.py:359-362), HIP -> RuntimeError.
 */
#ifndef TMA_H
#define TMA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMA_VERSION 227

enum { TMA_OK = 0, TMA_ERR_INVALID = 1, TMA_ERR_UNKNOWN_TASK = 2, TMA_ERR_HIP = 3 };

/* task ids (backend/mlagents/registry.py:52-116,225-240) */
enum { TMA_TASK_BASIC = 0, TMA_TASK_GRIDWORLD = 1, TMA_TASK_BALL3D = 2, TMA_TASK_PUSH = 3, TMA_TASK_CRAWLER = 4, TMA_TASK_WALLJUMP = 5, TMA_TASK_BICYCLE = 6, TMA_TASK_BRICKBREAK = 7, TMA_TASK_GLIDER = 8,
       TMA_TASK_ANT = 9, /* the reference's `ant` shapes (Ant-v5: 105 observations, 8 torques; envs.py:274-277) on the build's chain dynamics; CRAWLER = BASELINE.json's 172 / 20 shape */
       TMA_NUM_TASKS = 10 };

/* dtype of the `actions` buffer handed to tma_env_step */
enum { TMA_ACT_I32 = 0, TMA_ACT_I64 = 1, TMA_ACT_F32 = 2 };

/* episode k of (global) env i is reset with numpy-legacy seed  base + i + k * TMA_EP_STRIDE  (mod 2^32);
 * k = 0 is the reference's `seed + rank` (backend/mlagents/training.py:80,84). */
#define TMA_EP_STRIDE (1u << 20)

int tma_version(void);
const char *tma_last_error(void);

/* ---- task metadata: spaces declared by make_*_env (backend/mlagents/envs.py:35-44,162-199,274-277) ---- */
int tma_task_id(const char *name, int *task_out);
int tma_task_obs_dim(int task);           /* 21 / 4 / 6 / 4 / 172 / 4 / 7 / 45 / 16 / 105 */
int tma_task_num_actions(int task);       /* Discrete(n); 0 for a Box action space */
int tma_task_act_dim(int task);           /* Box action dim (crawler: 20, ant: 8), else 1 */
int tma_task_state_dim(int task);         /* doubles per env in the flat get/set_state layout */
int tma_task_max_episode_steps(int task); /* 50 / 100 / 200 / 120 / 1000 / 150 / 2000 / 2000 / 4000 / 1000 */

/* ---- vector env: replaces make_vector_env + DummyVecEnv + Monitor + LegacySingleAgentGymAdapter +
 *      the task step()/reset() (backend/mlagents/training.py:71-89; backend/mlagents/envs.py:30-159;
 *      backend/examples/{gridworld.py:40-95, ball3d.py:47-113, push.py:39-125, walljump.py:40-98, bicycle.py:40-141,
 *      brick_break.py:39-131, glider.py:55-265}) ---- */
typedef struct tma_env tma_env;

/* env_offset = global index of this shard's env 0 (data-parallel sharding); ring_depth = look-ahead of
 * pre-drawn reset states per env (>= 2; the MT19937 reset states of future episodes are produced by a
 * separate refill kernel every ring_depth steps). */
int tma_env_create(int task, int64_t num_envs, int device, uint32_t seed_base, uint32_t env_offset, int ring_depth,
                   tma_env **out);
/* destroy drains the device; the handle's device blocks (up to 64 MiB each, 512 MiB per process) are kept for the next tma_env_create that asks
 * for the same sizes -- the callers this replaces build and close a vector env per training run and per evaluation */
int tma_env_destroy(tma_env *h);
/* VecEnv.seed(seed): env i -> seed + i at the next reset (SB3 DummyVecEnv) */
int tma_env_seed(tma_env *h, uint32_t seed_base);
/* VecEnv.reset(): every env starts episode 0;  obs_out f32[num_envs][obs_dim] */
int tma_env_reset(tma_env *h, float *obs_out, void *stream);
/*
 * VecEnv.step_wait() for n_steps consecutive vector steps in ONE launch (n_steps = 1 is the plain
 * VecEnv.step).  actions: [n_steps][num_envs] (I32/I64) or [n_steps][num_envs][act_dim] (F32); if NULL the
 * counter-based tape a(i,t) = mix32(tape_seed, global_i, tape_t0 + s) % n_actions is generated on device.
 * Outputs are [n_steps][num_envs][...]; obs is the post-auto-reset observation (what DummyVecEnv
 * returns), term_obs the pre-reset observation where done (info["terminal_observation"]), ep_ret/ep_len the
 * Monitor episode sum/length where done (else 0).  rew/term/trunc/term_obs/ep_ret/ep_len may be NULL.
 * n_steps must not exceed tma_env_steps_until_refill().
 */
int tma_env_step(tma_env *h, const void *actions, int action_dtype, uint32_t tape_seed, uint32_t tape_t0, int n_steps,
                 float *obs_out, float *rew_out, uint8_t *term_out, uint8_t *trunc_out, float *term_obs_out,
                 double *ep_ret_out, int32_t *ep_len_out, void *stream);
/* Seam S1 (backend/mlagents/envs.py:125-152): the reference's single env returns `float(reward)` of the value the task computed in float64
 * (Basic 0.09000000000000001, Bicycle / BrickBreak / Glider rewards out of float64 physics); `rew_out` carries its float32 rounding, which is
 * what SB3's VecEnv keeps.  tma_env_set_reward64(env, plane, capacity): every tma_env_step launched afterwards ALSO stores the float64 reward
 * at plane[k * num_envs + i] (device memory owned by the caller, `capacity` doubles >= num_envs; a step call with n_steps * num_envs beyond it
 * is refused with TMA_ERR_INVALID); NULL turns it off -- the caller does that before it frees the plane.  The fused rollout kernels
 * (tma_rollout_collect) do not write it: they replace SB3's float32 buffer, not the Gymnasium single-env surface.  (ABI 208: the capacity.) */
int tma_env_set_reward64(tma_env *env, double *plane, int64_t capacity);
/* `reps` consecutive single-step launches with the same action buffer and output planes, issued from native code with no
 * host-language round trip in between (launch-latency measurements; semantics = calling tma_env_step `reps` times) */
int tma_env_step_repeat(tma_env *h, const void *actions, int action_dtype, int reps, float *obs_out, float *rew_out, uint8_t *term_out,
                        uint8_t *trunc_out, float *term_obs_out, void *stream);
int tma_env_steps_until_refill(tma_env *h, int *out);
/* engine options; "refill_small_window" = 1 shortens the register-resident MT19937 window so tests exercise the
 * general in-memory generator that takes over when rejection sampling needs more outputs */
int tma_env_set_option(tma_env *h, const char *key, int64_t value);
/* re-draw the reset states consumed since the last refill (exact numpy MT19937 legacy stream) */
int tma_env_refill(tma_env *h, void *stream);
/* flat float64 state [num_envs][state_dim] in the oracle's layout (state injection for parity tests;
 * also BasicMoveToGoalEnv.reset(options={"position": p}), backend/mlagents/envs.py:54-57) */
int tma_env_get_state(tma_env *h, double *state_out, void *stream);
int tma_env_set_state(tma_env *h, const double *state_in, void *stream);
int tma_env_episode_index(tma_env *h, uint32_t *out, void *stream);
/* Optional per-episode Monitor log (SB3 Monitor writes one `r,l,t` row per finished episode: reference training.py:85-86).  capacity > 0
 * allocates a device log of that many records and turns logging on in every step / rollout kernel; 0 turns it off.  Synchronises the
 * device.  tma_env_pop_episode_log copies up to max_records records (return, length, env index; in the order the kernels appended them)
 * to HOST memory, reports how many were stored (*n_stored) and how many episodes ended since the last pop (*n_seen >= *n_stored when the
 * log overflowed), and empties the log.  Synchronises `stream`. */
int tma_env_episode_log(tma_env *env, int64_t capacity);
int tma_env_pop_episode_log(tma_env *env, double *ret_host, int32_t *len_host, int32_t *env_host, int64_t max_records, int64_t *n_stored,
                            int64_t *n_seen, void *stream);
/* SB3 Monitor file rows (backend/mlagents/training.py:85-86: every env is wrapped in Monitor(env, filename), which appends one `r,l,t` line
 * per finished episode): appends n lines "round(ret, 6),len,round(t, 6)" to `path`, printed like Python prints those values.  HOST arrays,
 * no GPU work, thread-safe for distinct paths: the Python layer calls it from a writer thread. */
int tma_monitor_append_rows(const char *path, const double *ret, const int32_t *len, const double *t, int64_t n);
/* Monitor aggregate since the last call: out[0]=sum of episode returns, out[1]=sum of lengths, out[2]=count.
 * Synchronises `stream`. */
int tma_env_pop_episode_stats(tma_env *h, double *out3_host, void *stream);
/* Empty the episode log and the Monitor aggregate ordered on `stream` (two hipMemsetAsync), without reading them and without synchronising:
 * what a deterministic evaluation does before its first chunk (SB3's evaluate_policy starts from fresh Monitor state by construction,
 * backend/mlagents/training.py:240-247) -- whatever an earlier user of the env left, kernels launched on `stream` after this call start from zero. */
int tma_env_clear_episode_log(tma_env *env, void *stream);
/* Two-phase pop for a training loop that keeps the GPU busy across iterations (round 4; the reference's Monitor / logger run on the host
 * between rollouts, training.py:85-86,152-161 -- here they must not sit between two GPU iterations).  tma_env_detach_episode_log: HOST-side
 * swap of the buffer set handed to kernels at launch -- kernels launched BEFORE the call wrote their Monitor aggregates and episode records
 * into the set that is now detached, later launches write into the other, empty set; no stream is touched.  tma_env_pop_detached_episode_log:
 * tma_env_pop_episode_log + tma_env_pop_episode_stats of the detached set on any stream ordered behind those earlier kernels (a side stream
 * behind an event); empties it; synchronises only `stream`.  One detached set at a time (TMA_ERR_INVALID otherwise). */
int tma_env_detach_episode_log(tma_env *env);
int tma_env_pop_detached_episode_log(tma_env *env, double *ret_host, int32_t *len_host, int32_t *env_host, int64_t max_records, int64_t *n_stored,
                                     int64_t *n_seen, double *stats3_host, void *stream);

/* ---- GAE: replaces SB3 RolloutBuffer.compute_returns_and_advantage (3P, constructed at
 *      backend/mlagents/training.py:150; hyper-parameters training.py:383-384).  All [T][N] f32. ---- */
int tma_gae(const float *rewards, const float *values, const float *episode_starts, const float *last_values,
            const uint8_t *dones, double gamma, double gae_lambda, int T, int64_t N, float *adv_out, float *ret_out,
            void *stream);
/* SB3 `train/explained_variance` (PPO.train: explained_variance(rollout_buffer.values.flatten(), rollout_buffer.returns.flatten())):
 * out_dev[0] = 1 - Var(returns - values) / Var(returns) over the n = T * N floats of the two planes (population variances), NaN where
 * Var(returns) == 0.  ABI 210.  Accumulated in float64 as (count, mean, M2) triples -- Welford per thread, Chan's merge over lanes, waves and
 * blocks in a fixed order, plain stores and no floating-point atomics -- so the result is bit-identical from run to run and returns with a
 * large mean do not cancel (SB3 takes np.var of the float32 arrays: DESIGN.md section 7).  `scratch`: TMA_EV_SCRATCH_DOUBLES doubles of device
 * memory the two launches use between them; out_dev: one double of device memory.  Nothing is synchronised: the caller copies out_dev
 * stream-ordered. */
#define TMA_EV_SCRATCH_DOUBLES 1536
int tma_explained_variance(const float *values, const float *returns, int64_t n, double *scratch, double *out_dev, void *stream);

/* ---- actor-critic MLP + PPO update: replaces the SB3 objects PPO("MlpPolicy", env, **kwargs) builds at
 *      backend/mlagents/training.py:150 (policy_kwargs net_arch pi/vf = [H, H], training.py:363-365; hyper-parameters
 *      training.py:377-390) and model.learn() drives at training.py:166-170.  Third-party semantics: SURVEY.md App. C. ---- */
typedef struct {
    int obs_dim;    /* D */
    int hidden;     /* H: two hidden layers of width H (tanh, or `activation` below) for both the policy and the value net (multiple of 64) */
    int act_dim;    /* Discrete(n): n (2..16); Box: action dimension (1..32) */
    int continuous; /* 0: Categorical head; 1: DiagGaussian head with a state-independent log_std */
    int mfma_dtype; /* 0: f32 MFMA everywhere (parity mode, every hidden width); 1: bf16 MFMA operands with f32 master
                       weights and f32 accumulation for the hidden-layer and head GEMMs (hidden = 128 / 192 / 256 only:
                       BASELINE.json configs[2] "PPO MLP(256,256) bf16").  Rollout and update use the same forward code.
                       2 (round 5, opt-in): the f32 UPDATE of a Discrete 256 x 256 policy (the reference's default net,
                       backend/mlagents/training.py:363-365; up to 32 observations) on the bf16 MFMA with every operand as three bf16
                       terms and the six products of order <= 2 -- f32-class accuracy (2^-21 against float64, the exact-f32 MFMA's own
                       figure) at ~1.8x the f32 matrix pipe; rollouts, evaluation and small minibatches run the exact-f32 kernels. */
    int device;     /* HIP device the parameter / rollout / workspace buffers live on: every tma_policy_* / tma_ppo_* call makes it
                       the calling thread's current device first (callers may be worker threads: backend/main.py:152
                       asyncio.to_thread).  -1: keep whatever device is current on the calling thread. */
    int activation; /* ABI 220: the hidden layers' non-linearity (SB3 policy_kwargs activation_fn).  TMA_ACT_TANH (0): every kernel family;
                       TMA_ACT_RELU (1): h = z > 0 ? z : 0, derivative h > 0 ? 1 : 0 (torch's rule: 0 at z == 0), on the generic
                       one-wave-per-tile kernels only (forward, minibatch gradient, phase (a) of the VJP) -- the tuned families, the
                       persistent epoch kernels and the fused rollout chunks stay tanh-only and a ReLU policy never reaches them.
                       mfma_dtype must be 0 with it.  Parameter count, offsets and workspace sizes do not depend on it. */
} tma_policy_dims;
#define TMA_ACT_TANH 0
#define TMA_ACT_RELU 1

/* parameter buffer = n_total floats: [0, n_trainable) trainable, [in][out] layout, order
 * pi.W1 pi.b1 pi.W2 pi.b2 pi.W3(action_net) pi.b3 vf.W1 vf.b1 vf.W2 vf.b2 vf.W3(value_net) vf.b3 [log_std];
 * the rest are [out][in] copies maintained by tma_policy_sync / tma_ppo_adam_step. */
int tma_policy_param_count(const tma_policy_dims *d, int64_t *n_trainable, int64_t *n_total);
int tma_policy_param_offsets(const tma_policy_dims *d, int32_t *out13);
int tma_policy_sync(float *params, const tma_policy_dims *d, void *stream);
/* ActorCriticPolicy.forward(obs, deterministic): actions i32[n] (Discrete) or f32[n][act_dim] (Box, unclipped),
 * values f32[n], log_prob f32[n].  Sampling uses the counter-based stream (rng_seed, env_offset + row, rng_step). */
int tma_policy_act(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, uint32_t rng_seed, uint32_t rng_step,
                   uint32_t env_offset, int deterministic, void *actions_out, float *values_out, float *logp_out, void *stream);
/* tma_policy_act for step t plus tma_policy_bootstrap for step t-1 in one launch (prev_* may be NULL) */
int tma_policy_act_bootstrap(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, uint32_t rng_seed, uint32_t rng_step,
                             uint32_t env_offset, void *actions_out, float *values_out, float *logp_out, const float *prev_terminal_obs,
                             const uint8_t *prev_truncated, double gamma, float *prev_rewards_inout, void *stream);
/* ActorCriticPolicy.evaluate_actions(obs, actions) (ABI 210): values f32[n], log_prob f32[n] and entropy f32[n] of GIVEN actions -- i32[n]
 * (Discrete) or f32[n][act_dim] (Box, unclipped: the rollout buffer's layout).  Any output may be NULL, not all three.  The kernels are the
 * ones tma_policy_act runs (same specialisation for a shape, same layer code and k order, same grid caps; tma_debug_last_dispatch reports
 * the same TMA_DISPATCH_FWD_* id): `values` is bit-identical to tma_policy_act's, and so is `log_prob` where `actions` are the ones it drew.
 * Categorical: log_softmax at the action, -sum p log p.  DiagGaussian: sum_j -d^2 / (2 sigma^2) - log sigma - log(2 pi) / 2 and
 * sum_j 1/2 + log(2 pi) / 2 + log sigma.  A Discrete action outside [0, act_dim) is only ever compared with column indices (it never
 * addresses memory): that row's log_prob is NaN, its value and entropy are those of any other row.  mfma_dtype 2 policies take the exact-f32
 * kernels.  Bad dims, null params / obs / actions, n < 1 and three NULL outputs are refused (TMA_ERR_INVALID) before any HIP call. */
int tma_policy_evaluate_actions(const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                                float *values_out, float *logp_out, float *entropy_out, void *stream);
/* VJP of tma_policy_evaluate_actions with respect to the trainable parameters (ABI 215): what torch autograd computes behind SB3's
 * ActorCriticPolicy.evaluate_actions when a caller's own loss is back-propagated through it --
 *   grad_out[n_trainable] = sum_i  g_values[i] dV_i/dtheta + g_logp[i] dlogp_i/dtheta + g_entropy[i] dH_i/dtheta.
 * Any cotangent (f32[n]) may be NULL (= zeros), not all three.  grad_out is OVERWRITTEN (every element written; the caller need not zero it).
 * Parameter and gradient layout are tma_ppo_minibatch_grad's: the trainable prefix, [in][out] matrices, log_std last; `params` must be synced
 * (the [out][in] copies are read).  obs f32[n][D] dense; actions i32[n] (Discrete) or f32[n][act_dim] (Box) as in tma_policy_evaluate_actions;
 * a Discrete action outside [0, act_dim) is only ever compared with column indices: its one-hot is all zero and it never addresses memory.
 * mfma_dtype 0 and 2 (2 runs the exact-f32 code, as evaluate_actions does); mfma_dtype 1 (bf16) is refused: its forward rounds the operands and
 * an f32 backward would not be its derivative.  DETERMINISTIC: no float atomics; rows are walked in chunks (forward + input gradients of a
 * chunk into `workspace`, then output-stationary weight-gradient GEMMs over its rows in row order, added to grad_out chunk after chunk), so the
 * same inputs give the same bits on every run.  `workspace`: tma_policy_vjp_workspace_bytes(d, n) bytes of device memory, at most 256 MB for
 * every accepted shape whatever n (0 + message for refused dims / n < 1).  TMA_VJP_CHUNK_ROWS (environment, read on every call; a multiple of 16,
 * at least 16): a chunk length below the default.  Bad dims, null params / obs / actions / grad_out, n < 1, three NULL cotangents and a
 * workspace below what the bytes function reports are refused (TMA_ERR_INVALID) before any HIP call. */
int64_t tma_policy_vjp_workspace_bytes(const tma_policy_dims *d, int64_t n);
int tma_policy_evaluate_actions_backward(const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                                         const float *g_values, const float *g_logp, const float *g_entropy, float *grad_out, void *workspace,
                                         int64_t workspace_bytes, void *stream);
/* ActorCriticPolicy.get_distribution(obs) (ABI 218): the policy net's head BEFORE any distribution arithmetic -- head_out f32[n][act_dim], dense
 * (row stride act_dim): the raw logits (action_net's output, not normalised) of a Discrete policy, the mean of a Box policy -- and, where
 * values_out is not NULL, values f32[n].  The kernels are the ones tma_policy_act runs, in a further mode (same specialisation for a shape, same
 * layer code and k order, same grid caps; tma_debug_last_dispatch reports the same TMA_DISPATCH_FWD_* id): `values` is bit-identical to
 * tma_policy_act's, a Box head_out to the actions of tma_policy_act(deterministic = 1), and the first maximal column of a Discrete head_out row is
 * its deterministic action.  The head tile is stored coalesced; rows behind n are never stored.  Every mfma_dtype: 1 gives the bf16 kernels' own
 * head, 2 runs the exact-f32 code.  Bad dims, null params / obs / head_out and n < 1 are refused (TMA_ERR_INVALID) before any HIP call. */
int tma_policy_head(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, float *head_out, float *values_out, void *stream);
/* VJP of tma_policy_head with respect to the trainable parameters (ABI 218): what torch autograd computes behind a loss on SB3's
 * policy.get_distribution(obs) (KL between policies, distillation) --
 *   grad_out[n_trainable] = sum_i sum_j g_head[i][j] dhead_ij/dtheta + sum_i g_values[i] dV_i/dtheta.
 * g_head f32[n][act_dim] (dense) and g_values f32[n] may each be NULL (= zeros), not both.  grad_out is OVERWRITTEN, every element -- the log_std
 * segment of a Box policy with zeros: the head does not depend on log_std (a distribution's dependence on it is the caller's own arithmetic).
 * Parameter layout, `workspace` (tma_policy_vjp_workspace_bytes(d, n) bytes), chunking, TMA_VJP_CHUNK_ROWS and the determinism contract are
 * tma_policy_evaluate_actions_backward's: the same two launches per chunk, the first taking a row's head cotangent from g_head instead of forming
 * it from three cotangents, the second unchanged.  mfma_dtype 1 (bf16) is refused as there.  Bad dims, null params / obs / grad_out, n < 1, two
 * NULL cotangents and a workspace below what the bytes function reports are refused (TMA_ERR_INVALID) before any HIP call. */
int tma_policy_head_backward(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, const float *g_head, const float *g_values,
                             float *grad_out, void *workspace, int64_t workspace_bytes, void *stream);
/* The two VJPs above with the gradient with respect to the OBSERVATIONS as a second output (ABI 222): what torch autograd computes behind a torch
 * module in front of the policy (a learned encoder) or behind a loss differentiated with respect to a frozen policy's input (saliency, FGSM / PGD,
 * a teacher's dKL/dobs) --
 *   grad_obs[i][k] = sum_n dz1_pi[i][n] W1_pi[n][k] + sum_n dz1_vf[i][n] W1_vf[n][k],   dz1: row i's cotangent at the first layer's pre-activation.
 * grad_params f32[n_trainable] and grad_obs f32[n][obs_dim] (dense) may each be NULL, not both.  With grad_obs NULL the call IS the ..._backward
 * call above: the same launches, the same bits.  With grad_params NULL (a frozen policy) the weight-gradient launch is skipped.  grad_obs is
 * OVERWRITTEN, exactly n * obs_dim floats (a row whose cotangents are all zero gets zeros), by a third launch per chunk behind the other two:
 * one wave per 16-row tile on the f32 MFMA, no reduction over rows, one accumulator chain per element in an order that depends on `hidden`
 * alone -- a row's gradient has the same bits whatever the batch around it, the chunk length, or whether grad_params is asked for.  grad_params
 * has the bits of the ..._backward call whether or not grad_obs is asked for.  grad_obs needs no alignment beyond a float's.  Workspace, chunking,
 * TMA_VJP_CHUNK_ROWS and every refusal are those of the ..._backward calls (grad_params itself may be NULL here); also refused (TMA_ERR_INVALID,
 * before any HIP call): both outputs NULL, grad_obs overlapping obs (byte ranges of n * obs_dim * 4) and grad_obs overlapping the workspace. */
int tma_policy_evaluate_actions_vjp(const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                                    const float *g_values, const float *g_logp, const float *g_entropy,
                                    float *grad_params /* [n_trainable] or NULL */, float *grad_obs /* [n][obs_dim] or NULL */,
                                    void *workspace, int64_t workspace_bytes, void *stream);
int tma_policy_head_vjp(const float *params, const tma_policy_dims *d, const float *obs, int64_t n,
                        const float *g_head, const float *g_values,
                        float *grad_params, float *grad_obs, void *workspace, int64_t workspace_bytes, void *stream);
/* ActorCriticPolicy.predict_values */
int tma_policy_values(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, float *values_out, void *stream);
/* collect_rollouts timeout bootstrap: rewards[i] += gamma * V(terminal_obs[i]) where truncated[i] */
int tma_policy_bootstrap(const float *params, const tma_policy_dims *d, const float *terminal_obs, const uint8_t *truncated, int64_t n,
                         double gamma, float *rewards_inout, void *stream);

typedef struct {
    const float *obs;       /* [T][N][D]                                  RolloutBuffer.observations */
    const void *actions;    /* i32 [T][N] (Discrete) or f32 [T][N][A] (Box)              .actions    */
    const float *log_probs; /* [T][N]                                                     .log_probs  */
    const float *advantages;
    const float *returns;
    int T;
    int64_t N;
    const float *packed;    /* optional, NULL = absent: [T][N][tma_ppo_packed_floats / (T*N)] sample records {obs (padded to a multiple of 4), log_prob,
                               advantage, action bits, return} written by tma_ppo_pack_samples from the five planes above.  With it the H = 64
                               gradient kernel reads ONE record (one 64-byte line) per sample and net instead of gathering from five planes.
                               Results are bit-identical with and without it. */
} tma_rollout;

typedef struct {
    const int64_t *indices; /* optional explicit permutation of the env-major flat index f = i*T + t (SB3 swap_and_flatten);
                               NULL -> on-device Feistel permutation keyed by (perm_seed, perm_epoch) */
    uint32_t perm_seed, perm_epoch;
    int64_t start, count;   /* this minibatch = permuted rows [start, start + count) */
    int64_t prepared_batch; /* 0: self-contained call.  > 0: tma_ppo_epoch_prepare ran on this workspace for the same rollout view,
                               (perm_seed, perm_epoch) and this batch size, start is a multiple of it -- the per-minibatch advantage
                               pass is skipped and the cached sample offsets / advantage partials are used */
    int64_t stats_count;    /* 0: advantages are normalised with the mean / unbiased std of this minibatch's `count` rows.
                               > 0 (data-parallel runs, prepared epochs only): the workspace partials of this minibatch were replaced
                               by sums over the GLOBAL minibatch of stats_count rows (tma_ppo_epoch_adv_sums) -- every rank then
                               normalises with the same global mean / std, as one SB3 run over the concatenated batch would */
} tma_minibatch;

typedef struct {
    double clip_range, ent_coef, vf_coef;
    int normalize_advantage;
} tma_ppo_hparams;

/* Sample records for tma_rollout.packed: floats the plane needs for this policy shape and T x N samples (0: the shape has no use for it --
 * today: hidden 64, Discrete head, <= 8 observations), and the pass that fills it (once per rollout, after the advantages and returns exist). */
int64_t tma_ppo_packed_floats(const tma_policy_dims *d, int T, int64_t N);
int tma_ppo_pack_samples(const tma_rollout *rb, const tma_policy_dims *d, float *packed_out, void *stream);
/* bytes of the update workspace for a policy shape (loss-stat slots, norm partials, partial-gradient slabs, sample-offset cache;
 * bf16 layouts with 33..64 or 161..192 observations: + a dz1 cache of 2 * 262144 * hidden bf16 for the dW1 launch; f32 layouts with
 * hidden 128/192/256 and 161..176 observations: the same in f32) */
int64_t tma_ppo_workspace_bytes(const tma_policy_dims *d);
/* PPO.train inner loop body up to loss.backward(): accumulates d(loss)/d(params) into grad[n_trainable] (caller zeroes it
 * once; tma_ppo_adam_step re-zeroes it) and loss statistics into the workspace. */
int tma_ppo_minibatch_grad(const float *params, const tma_policy_dims *d, const tma_rollout *rb, const tma_minibatch *mb,
                           const tma_ppo_hparams *hp, float *grad, void *workspace, void *stream);
/* Once per epoch (optional): sample offsets of the whole permutation and the advantage (sum, sum of squares) partials of every
 * minibatch [k*batch_size, (k+1)*batch_size) in one launch, instead of one small launch in front of every minibatch gradient.
 * epoch->start / count describe the whole pass (0, T*N).  Needs T*N <= 2^22 and batch_size >= 256, else TMA_ERR_INVALID. */
int tma_ppo_epoch_prepare(const tma_rollout *rb, const tma_minibatch *epoch, int64_t batch_size, const tma_policy_dims *d, void *workspace,
                          void *stream);
/* Data-parallel advantage statistics ("12-byte all-reduce for global advantage mean/var"), for an epoch that
 * tma_ppo_epoch_prepare just prepared on this workspace with the same batch_size over `total` = T*N samples.
 * direction 0 (export): sums[k] = {sum, sum of squares} of minibatch k's advantages (double[n_minibatches][2], device memory), folded
 * from the workspace partials in a fixed order.  The caller all-reduces (sum) that buffer over the ranks -- ONE collective of
 * 16 * n_minibatches bytes per epoch -- and hands it back with direction 1 (import), which makes it the workspace's partials;
 * the epoch's minibatches are then run with tma_minibatch.stats_count = global row count. */
int tma_ppo_epoch_adv_sums(void *workspace, const tma_policy_dims *d, int64_t batch_size, int64_t total, double *sums, int direction,
                           void *stream);
/* clip_grad_norm_(max_grad_norm) + Adam.step() (+ refresh of the [out][in] copies).  grad_scale multiplies the gradient
 * first (1/world_size after an all-reduce(sum)). */
int tma_ppo_adam_step(float *params, float *grad, float *exp_avg, float *exp_avg_sq, const tma_policy_dims *d, int64_t step, double lr,
                      double beta1, double beta2, double eps, double max_grad_norm, double grad_scale, void *workspace, void *stream);
/* Same update for the single-GPU case where `grad` is exactly what the LAST tma_ppo_minibatch_grad on this workspace produced
 * (no all-reduce, no accumulation over several minibatches; last_count = that minibatch's sample count): the gradient norm is taken
 * from partial sums the gradient reduction already left in the workspace and the derived copies are written by the optimizer kernel
 * itself (one launch instead of three).  Falls back to tma_ppo_adam_step(grad_scale = 1) for shapes without that fast path. */
int tma_ppo_adam_step_local(float *params, float *grad, float *exp_avg, float *exp_avg_sq, const tma_policy_dims *d, int64_t step, double lr,
                            double beta1, double beta2, double eps, double max_grad_norm, void *workspace, void *stream, int64_t last_count);
/* One whole epoch of PPO.train on ONE GPU in a single call: [tma_ppo_epoch_prepare] + for every minibatch of batch_size rows of the
 * (perm_seed, perm_epoch) permutation: tma_ppo_minibatch_grad + tma_ppo_adam_step_local, issued natively with no host-language round trip
 * in between (at the reference's literal batch_size = 256 and 4096 envs an epoch is 16 384 optimizer steps: backend/mlagents/training.py:379).
 * first_step = Adam step index of the epoch's first minibatch (>= 1); grad must be zero on entry and is zero on return.  On H = 64 fast-path
 * policies with every minibatch >= 256 rows the optimizer step of minibatch k runs in the prologue of gradient launch k + 1 (two launches per
 * minibatch; the state ping-pongs between the caller's buffers and a copy in the workspace and ends in the caller's buffers; TMA_NO_ADAM_FOLD=1
 * in the environment: one optimizer launch per minibatch).  Bit-identical to the
 * per-minibatch calls -- except on H = 64 policies at batch_size = 256 with T*N a multiple of it, where the epoch runs as ONE persistent
 * launch (csrc/tma_h64p.hip: weights in LDS, Adam moments in registers, eight workgroups of one XCD exchanging partial gradients through
 * the L2): same gradient sums and Adam arithmetic, the clip norm's f64 sum in another fixed order (parameters agree to the last bit or
 * two) -- and, since ABI 208, on the reference's DEFAULT policy (two 256 x 256 tanh nets, f32 weights: mfma_dtype 0 or 2; Discrete head of
 * <= 16 actions, <= 32 observations; backend/mlagents/training.py:363-365) at batch_size = 256, where the epoch is ONE persistent launch of
 * csrc/tma_h256p.hip: each net on the 32 CUs of one XCD as 4 row groups x 8 column slices, weights of a slice in LDS, Adam moments in
 * registers, four same-XCD exchanges of activations and partial gradients per optimizer step; its sums have their own fixed order, so it is
 * run-to-run bit-identical and equal to the per-minibatch launches to rounding (2e-6 on the parameters after three epochs; 18.9 us per
 * optimizer step where the three launches take 34.2).  TMA_NO_PERSIST=1 in the environment selects the per-minibatch launches
 * (TMA_NO_PERSIST256=1: for the 256-wide kernel only).  Should a persistent kernel fail to place or synchronise its workgroups (eight
 * resident on one XCD; 32 on each of two for the 256-wide one) it commits nothing; this call notices (it waits for the persistent launch and
 * reads one status word back), restores its snapshot, re-runs the epoch through the per-minibatch launches and counts the event
 * (tma_ppo_persist_fallbacks). */
int tma_ppo_train_epoch_local(float *params, const tma_policy_dims *d, const tma_rollout *rb, uint32_t perm_seed, uint32_t perm_epoch,
                              int64_t batch_size, const tma_ppo_hparams *hp, float *grad, float *exp_avg, float *exp_avg_sq, int64_t first_step,
                              double lr, double beta1, double beta2, double eps, double max_grad_norm, void *workspace, void *stream);
/* `n_epochs` consecutive epochs (permutations perm_epoch0, perm_epoch0 + 1, ...; optimizer steps first_step ...) in one call.  Where a persistent
 * epoch kernel takes the shape (batch_size 256: H = 64 fast-path layouts, and the reference's default 256 x 256 f32 policy with a Discrete head
 * and <= 32 observations) and n_epochs * T * N sample offsets fit the workspace cache (2^22), ALL the epochs run as ONE launch -- the
 * reference's own 1- and 8-env schedules are 4 and 32 optimizer steps per epoch, where a launch per epoch is mostly launch; otherwise (and
 * when such a launch cannot place its workgroups) exactly tma_ppo_train_epoch_local per epoch.  Same results either way.
 * ABI 212, H = 64 fast-path policies at minibatches of more than 2 048 rows (the eight-wave gradient kernel): the epochs of the call are ONE
 * chain of gradient launches.  There is no tma_ppo_epoch_prepare launch: one adv_partial_kernel launch over the call's first minibatch, then
 * gradient launch k leaves the sample offsets and advantage partials of minibatch k + 1 -- at an epoch's end: of minibatch 0 of the next
 * epoch -- where tma_ppo_epoch_prepare would have (its value-net workgroups do it once their own work is stored; a tail minibatch of
 * <= 2 048 rows, before and behind it, gets a launch over that minibatch alone).  Every epoch ends in the ordinary optimizer launch.
 * Bit-identical to the per-epoch sequence, which TMA_NO_PREP_FOLD=1 in the environment (read per call) selects. */
int tma_ppo_train_epochs_local(float *params, const tma_policy_dims *d, const tma_rollout *rb, uint32_t perm_seed, uint32_t perm_epoch0, int n_epochs,
                               int64_t batch_size, const tma_ppo_hparams *hp, float *grad, float *exp_avg, float *exp_avg_sq, int64_t first_step,
                               double lr, double beta1, double beta2, double eps, double max_grad_norm, void *workspace, void *stream);
/* Test aid (ABI 212): advantage pre-passes of the calling thread's last tma_ppo_train_epoch_local / tma_ppo_train_epochs_local call -- how many
 * rode on a gradient launch (*folded_out) and how many were launches of their own (*standalone_out: a tma_ppo_epoch_prepare launch over
 * a whole epoch counts as one).  No GPU work. */
int tma_debug_last_prep_fold(int *folded_out, int *standalone_out);
/* One epoch of PPO.train on ONE RANK of a data-parallel job (env shards per GPU, one gradient all-reduce per
 * minibatch; the reference itself is one process, backend/mlagents/training.py:71-89,150): for every minibatch of batch_size local rows --
 * tma_ppo_minibatch_grad, then `allreduce(ctx, grad, n_trainable)` (the caller's collective: SUM over the ranks, in place, enqueued on
 * `stream` or ordered against it -- torch.distributed.all_reduce on the current stream does that; must return 0), then
 * clip_grad_norm_ + Adam on grad * grad_scale (1 / world size) -- issued natively, the collective being the only host-language call per
 * minibatch.  Bit-identical to tma_ppo_minibatch_grad / all-reduce / tma_ppo_adam_step(grad_scale) called in a loop.
 * prepared_batch: batch_size if the caller ran tma_ppo_epoch_prepare (+ tma_ppo_epoch_adv_sums) for this epoch, else 0;
 * stats_world: multiplier of a minibatch's row count for its advantage statistics (world size with global statistics, else 0 = local).
 * grad must be zero on entry and is zero on return. */
typedef int (*tma_allreduce_fn)(void *ctx, float *buffer, int64_t count);
int tma_ppo_train_epoch_dp(float *params, const tma_policy_dims *d, const tma_rollout *rb, uint32_t perm_seed, uint32_t perm_epoch,
                           int64_t batch_size, int64_t prepared_batch, int stats_world, const tma_ppo_hparams *hp, float *grad, float *exp_avg,
                           float *exp_avg_sq, int64_t first_step, double lr, double beta1, double beta2, double eps, double max_grad_norm,
                           double grad_scale, tma_allreduce_fn allreduce, void *ctx, void *workspace, void *stream);
/* ---- RCCL communicator owned by the library (round 4): the collective of tma_ppo_train_epoch_dp without a host-language hop.
 *      The reference has no distributed code (one process: backend/mlagents/training.py:71-89,150); north_star's only collective is the
 *      per-minibatch SUM of the flat f32 policy gradient over the GPUs of a node.
 * Rank 0 draws a unique id (128 opaque bytes, ncclGetUniqueId), the caller broadcasts it over whatever channel it has (the torch.distributed
 * process group it rendezvoused with: any backend), every rank then calls tma_comm_create (ncclCommInitRank; collective over the ranks;
 * device < 0: the calling thread's current device).  tma_comm_allreduce: in-place SUM of `count` elements (dtype 0 = f32, 1 = f64) enqueued
 * on `stream` -- kernels queued on that stream before / after it are ordered before / after the collective, nothing else is needed.
 * tma_comm_allreduce_cb has the tma_allreduce_fn signature: pass it to tma_ppo_train_epoch_dp with the communicator as ctx (after
 * tma_comm_bind_stream(comm, the stream given to the epoch call)) and a data-parallel epoch runs without leaving native code.
 * RCCL is bound at run time (dlopen librccl.so.1: inside a PyTorch process that is the copy PyTorch loaded); tma_comm_available() == 0 and
 * TMA_ERR_HIP from the other entries when it cannot be.  tma_comm_timing(comm, n): bracket the next n all-reduces with HIP events on their
 * stream; tma_comm_pop_timing waits for them and returns their durations in microseconds (bench.py dp_timing) and the number of
 * all-reduces issued so far. */
typedef struct tma_comm tma_comm;
int tma_comm_available(void);
int tma_comm_unique_id(unsigned char *id_out128);
int tma_comm_create(const unsigned char *id128, int world, int rank, int device, tma_comm **out);
int tma_comm_destroy(tma_comm *comm);
int tma_comm_bind_stream(tma_comm *comm, void *stream);
int tma_comm_allreduce(tma_comm *comm, void *buffer, int64_t count, int dtype, void *stream);
int tma_comm_allreduce_cb(void *ctx, float *buffer, int64_t count);
int tma_comm_timing(tma_comm *comm, int samples);
int tma_comm_pop_timing(tma_comm *comm, float *us_out, int capacity, int *n_out, int64_t *calls_out);
/* ---- Peer exchange (round 5, ABI 207): the same SUM as direct xGMI stores between the GPUs of ONE node (up to 8 ranks), for messages where a
 *      ring's 2 (world - 1) hops and the collective's own launch are the cost (the 64 x 64 policy's gradient is 37 KB, 320 times per headline
 *      iteration).  Every rank owns an inbox in fine-grained device memory that its peers map through a HIP IPC handle; a sender stores each
 *      32-bit payload word with the all-reduce's sequence number next to it as ONE 8-byte word into its slot of every inbox, a receiver reads
 *      the `world` slots of its own inbox (system-scope 8-byte loads, until every word carries the expected sequence number) and adds them in
 *      rank order -- the same order on every rank, so replicas stay bit-identical; no fence and no ordering between words is assumed
 *      (csrc/tma_p2p.h has the protocol and why two slot parities suffice).
 * Set-up: tma_comm_p2p_prepare(comm, max_words, ticket_out[128]) allocates the inbox (slots of max_words 8-byte words; an f32 element is one
 * word, an f64 element two) and writes a 128-byte ticket (the inbox's IPC handle, the PCI bus id of its device, a 64-bit identity of the host); the caller gathers the
 * `world` tickets over the channel it already has (rank order) and gives them to tma_comm_p2p_attach, which refuses (TMA_ERR_HIP, nothing
 * mapped) unless every peer runs on THIS host and its device is this rank's own or a visible one with peer access (switched on there).  A
 * receiver that does not get its words within the timeout raises the communicator's error flag and delivers NaN (never a sum of stale
 * words); every later exchange then fails at once (tma_comm_p2p_status.timed_out, checked by the caller behind its stream synchronisation);
 * tma_comm_p2p_enable(comm, 1) then routes every tma_comm_allreduce /
 * tma_comm_allreduce_cb whose message fits a slot through the exchange (larger ones keep RCCL), and tma_ppo_train_epoch_dp -- given
 * tma_comm_allreduce_cb and such a communicator -- FUSES it on its H = 64 path: the slab reduction stores the reduced gradient into the
 * peers' inboxes, the sum-of-squares pass in front of the optimizer step reads the sum: no collective launch in the minibatch chain at all.
 * tma_comm_create_p2p: a communicator WITHOUT an RCCL side (several ranks on one GPU, which RCCL does not allow: the one-GPU tests); its
 * all-reduces must fit the exchange.  A receiver that waits longer than TMA_P2P_TIMEOUT_S (default 120) for a peer's words raises a flag:
 * the all-reduce that was waiting returns NaN (ABI 208; never a sum of stale words), every later one fails with TMA_ERR_HIP,
 * tma_comm_p2p_status reports it -- nothing spins for ever.  tma_comm_timing brackets the RECEIVING kernel of an exchange (what the chain waits for once the sender kernel is done). */
int tma_comm_create_p2p(int world, int rank, int device, tma_comm **out);
int tma_comm_p2p_prepare(tma_comm *comm, int64_t max_words, unsigned char *ticket_out128);
int tma_comm_p2p_attach(tma_comm *comm, const unsigned char *tickets_world_x_128);
/* The same wiring for `world` communicators that live in ONE process (each created with tma_comm_create_p2p(world, r, device) and prepared
 * with the same max_words): peers[r] is rank r's communicator, its inbox is used directly.  For drivers that run several ranks as streams of
 * one process -- the tests run the exchange at the world sizes of a node (4, 8) on one GPU this way; a receiver spins on words another
 * rank's sender stores, so every rank needs a stream (hardware queue) of its own. */
int tma_comm_p2p_attach_local(tma_comm *comm, tma_comm *const *peers_world);
int tma_comm_p2p_enable(tma_comm *comm, int on);
int tma_comm_p2p_status(tma_comm *comm, int *enabled_out, int64_t *calls_out, int *timed_out_out, int64_t *slot_words_out);
int tma_comm_p2p_set_timeout(tma_comm *comm, double seconds); /* receivers of later exchanges give up after this long (set-up: a short one for the self-check) */
/* How many epochs of tma_ppo_train_epoch_local on this workspace fell back from the persistent launch to per-minibatch launches.  Synchronises `stream`. */
int tma_ppo_persist_fallbacks(void *workspace, int64_t *count_out, void *stream);
/* The minibatch order of the on-device permutation (the engine's stand-in for np.random.permutation in SB3's RolloutBuffer.get): writes, to
 * HOST memory, the env-major flat indices f = i*T + t of permuted rows [0, total) for (perm_seed, perm_epoch).  Minibatch m of size B is
 * rows [m*B, (m+1)*B).  Lets a caller reproduce or log the schedule; no GPU work. */
int tma_ppo_permutation(uint32_t perm_seed, uint32_t perm_epoch, int64_t total, int64_t *indices_out_host);
/* One minibatch of SB3's RolloutBuffer.get as dense device tensors (ABI 221): permuted rows [mb->start, mb->start + mb->count) of a rollout, in
 * ONE launch.  The gradient entries above gather their rows inside their kernels; this is for a caller who writes the update itself (a torch loss
 * on tma_policy_evaluate_actions / tma_policy_head and their VJPs) and needs the rows the engine's own epoch would have used.
 * Row selection is exactly the gradient kernels': mb->indices if given (device memory), else the on-device permutation (perm_seed, perm_epoch)
 * over T*N -- the env-major flat index f = i*T + t (SB3 swap_and_flatten), read from plane row t*N + i.  mb->prepared_batch and mb->stats_count
 * are ignored; rb->packed is never read.  `values`: the [T][N] plane of the rollout's value predictions (tma_rollout has none; may be NULL).
 * `d` supplies D, A and the head kind.  Outputs: obs_out f32[count][D], actions_out i32[count] (Discrete) or f32[count][A] (Box), the four
 * scalar planes f32[count]; any output pointer may be NULL and that plane is then skipped (old_values_out must be NULL when `values` is).
 * A pure copy: every output element has the bits of its source element.  No atomics, no workspace; the grid is capped and strides; every
 * offset is 64-bit.  Refused with TMA_ERR_INVALID before any HIP call: rb / d / mb NULL, bad dims, a source plane that is NULL while its
 * output is not, count < 1, start < 0, start + count > T*N, T*N >= 2^31. */
int tma_rollout_gather(const tma_rollout *rb, const float *values /* [T][N], may be NULL */, const tma_policy_dims *d, const tma_minibatch *mb,
                       float *obs_out /* [count][D] */, void *actions_out /* i32 [count] | f32 [count][A] */, float *old_values_out,
                       float *old_log_prob_out, float *advantages_out, float *returns_out, void *stream);

/* ---- replay buffer (ABI 224): SB3's ReplayBuffer / NStepReplayBuffer (3P: stable_baselines3/common/buffers.py, what the reference's DQN
 *      default keeps, backend/mlagents/training.py:343-360) as device planes -- written without a copy to the host, sampled as dense tensors in
 *      one launch.  DESIGN.md section 16. ---- */
/* The storage, caller-owned device memory as with tma_rollout: `capacity` rows R (>= 1) of `n_envs` envs N (>= 1).  obs_dim D and act_dim A in
 * [1, 4096]; a Discrete buffer (continuous = 0) stores one i32 per action and uses A nowhere.  The ring position and the fill state are NOT
 * device state: the host keeps them and passes them to each call. */
typedef struct tma_replay {
    float *obs;          /* [R][N][D]  the observation the action was chosen from */
    float *next_obs;     /* [R][N][D]  the observation it led to: the terminal observation where the step ended its episode */
    void *actions;       /* i32 [R][N] (Discrete) | f32 [R][N][A] (Box) */
    float *rewards;      /* [R][N] */
    uint8_t *terminated; /* [R][N] */
    uint8_t *truncated;  /* [R][N] */
    int capacity;
    int64_t n_envs;
    int obs_dim, act_dim, continuous;
} tma_replay;
/* ReplayBuffer.add for one vector step, in ONE launch: row `pos` of every plane.  Per env i:  obs[pos][i] = last_obs_inout[i];
 * next_obs[pos][i] = (term[i] | trunc[i]) ? term_obs[i] : step_obs[i]  (SB3's terminal_observation substitution in _store_transition);
 * actions i32[N] | f32[N][A], rewards f32[N] and the two flag rows u8[N] are copied;  then last_obs_inout[i] = step_obs[i], the post-reset
 * observation the next action is chosen from.  Why last_obs_inout: tma_env_step's outputs are overwritten by the next step, so the buffer's
 * owner keeps the current observation in memory of its own, and this launch keeps it current.  term_obs may be NULL ONLY IF THE CALLER
 * GUARANTEES THAT NO FLAG IS SET in term / trunc: next_obs is then step_obs for every env, whatever the flags say.  No atomics, no workspace;
 * the grid is capped and strides; every offset is 64-bit; nothing synchronises.  Refused with TMA_ERR_INVALID before any HIP call: rb NULL, bad
 * geometry, a NULL plane, a NULL argument other than term_obs, pos outside [0, R), last_obs_inout overlapping step_obs. */
int tma_replay_add(const tma_replay *rb, int64_t pos, float *last_obs_inout /* [N][D] */, const void *actions, const float *step_obs /* [N][D] */,
                   const float *rewards, const uint8_t *term, const uint8_t *trunc, const float *term_obs /* [N][D], may be NULL (above) */, void *stream);
/* ReplayBuffer.sample / NStepReplayBuffer.sample: draws `count` transitions and gathers them, in ONE launch.
 * `size`: the number of valid rows -- pos before the ring has wrapped, R afterwards; `newest`: the row last written, in [0, size).
 * Index draw, counter-based and reproducible (mix32 is the engine's stand-in for np.random.randint): for output row b
 *   t = (uint64(mix32(seed, b, draw)) * size) >> 32,   i = mix32(seed ^ 0x5EEDBA5E, b, draw) % N.
 * Bias: the multiply-shift maps 2^32 hash values onto `size` rows, so two rows' probabilities differ by at most 2^-32 (a relative size / 2^32);
 * the modulo's, N / 2^32 likewise.  Rows are drawn with replacement, as SB3 draws them.
 * The window of a draw, n = n_step: rows t, t+1, ... (mod R); step k is included while k < n; the window ends behind the first included step
 * whose terminated | truncated is set, and behind row `newest` (it never crosses the write head into older data).  With L >= 1 steps included:
 *   rewards_out   = sum_{k<L} gamma^k r_k, accumulated in float64 in k order (gamma^k by repeated float64 multiplication), rounded once to f32;
 *   next_obs_out  = next_obs of the last included step;   dones_out = its `terminated` as 0.0f / 1.0f (a time-out is not a done: SB3's
 *   handle_timeout_termination=True);   discounts_out = (float)gamma^L.
 * With n_step = 1 that is: rewards_out the stored reward, dones_out = terminated, discounts_out = (float)gamma.  obs_out f32[count][D],
 * actions_out i32[count] | f32[count][A] and next_obs_out f32[count][D] are pure copies: every element has the bits of its source element.
 * rows_out / envs_out i32[count] return (t, i).  Any output pointer may be NULL and is then skipped.  Observation rows move as dwords, as
 * float4 where D is a multiple of four and the bases are 16-byte aligned.  No atomics, no workspace; the grid is capped and strides.
 * Refused with TMA_ERR_INVALID before any HIP call: rb NULL, bad geometry, R * N >= 2^31, size outside [1, R], newest outside [0, size),
 * count < 1, n_step outside [1, 64], every output NULL, a NULL source plane (rewards, terminated, truncated; obs / actions / next_obs where their
 * output is asked for). */
int tma_replay_sample(const tma_replay *rb, int size, int newest, int n_step, double gamma, uint32_t seed, uint32_t draw, int64_t count,
                      float *obs_out, void *actions_out, float *next_obs_out, float *dones_out, float *rewards_out, float *discounts_out,
                      int32_t *rows_out, int32_t *envs_out, void *stream);
/* The epsilon-greedy action pick of SB3's DQN.predict on q f32[n][A] (dense, 2 <= A <= 16), e.g. a Discrete tma_policy_head output.  Per row:
 * u = (mix32(rng_seed, env_offset + row, rng_step) >> 8) * 2^-24;  u < (float)eps: action = mix32(rng_seed ^ 0xE9517EED, env_offset + row,
 * rng_step) % A;  else the first maximal column -- tma_policy_head's rule for the deterministic action; a NaN never wins, a row of NaNs gives 0.
 * The coin is per env (SB3 tosses one per predict call; the two coincide at n = 1).  actions_out i32[n].  Refused with TMA_ERR_INVALID before
 * any HIP call: q / actions_out NULL, n < 1, A outside [2, 16], eps outside [0, 1] or NaN. */
int tma_egreedy_actions(const float *q, int64_t n, int A, double eps, uint32_t rng_seed, uint32_t rng_step, uint32_t env_offset, int32_t *actions_out,
                        void *stream);

/* ---- DQN (ABI 225): SB3's DQN (3P: stable_baselines3/dqn/dqn.py; the reference's default for its Discrete tasks, backend/mlagents/training.py:343-360)
 *      -- csrc/tma_dqn.hip, DESIGN.md section 17.
 * The Q-network is the `pi.*` segment of a Discrete tma_policy_dims parameter buffer: pi.W1 ... pi.b3 is SB3's QNetwork features -> H -> H -> A; the
 * `vf.*` segment is never read.  The target net is a second buffer of the same layout (tma_policy_param_count floats).  Shapes: continuous 0,
 * mfma_dtype 0, activation tanh or ReLU, hidden 64 / 128 / 256, 2 <= act_dim <= 16, obs_dim <= 128.  Everything else is refused with
 * TMA_ERR_INVALID and a message before any HIP call, as are the NULLs and ranges each entry lists. */
/* The Q forward of the pi segment and the epsilon-greedy pick in ONE launch.  Per row exactly tma_egreedy_actions' rule and hash on this launch's
 * own Q row (same rng_seed / rng_step / env_offset meaning, first maximal column, a NaN never wins).  actions_out i32[n]; q_out f32[n][act_dim] or
 * NULL (skipped).  A workgroup of four waves per 16-row tile, the hidden columns split over the waves; the grid is capped and strides.  The Q of
 * a row has the bits tma_dqn_td_grad's online forward gives the same row (one device function), whatever the batch either came in.
 * Refused: NULL d / params / obs / actions_out, n < 1, eps outside [0, 1] or NaN. */
int tma_dqn_act(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, double eps, uint32_t rng_seed, uint32_t rng_step,
                uint32_t env_offset, int32_t *actions_out, float *q_out, void *stream);
/* The loss side of DQN.train for one batch, the inputs being what tma_replay_sample writes (obs f32[n][D], actions i32[n], next_obs f32[n][D], dones,
 * rewards, discounts f32[n]):
 *   y_i = rewards_i + (1 - dones_i) * discounts_i * max_a Q_target(next_obs_i, a)     (no gradient through y)
 *   delta_i = Q(obs_i, actions_i) - y_i;   loss = mean_i smooth_l1(delta_i), beta = 1: the cotangent clamp(delta_i, -1, 1) / n on column actions_i
 * and the gradient with respect to the pi segment.  grad_out[n_trainable] is OVERWRITTEN, the vf segment (and log_std: none, Discrete) with exact
 * zeros.  stats_out (device, may be NULL): three float64 -- sum_i smooth_l1(delta_i), sum_i Q(obs_i, actions_i), n -- so loss = stats[0] / stats[2].
 * q_out (may be NULL): f32[n][act_dim], the online Q the loss used (the bits tma_dqn_act gives the same rows).
 * `params` must be synced (the [out][in] copies of pi.W2 / pi.W3 are read); of target_params only the trainable [in][out] matrices are read.
 * An action outside [0, act_dim) is only ever compared with column indices (it never addresses memory): its cotangent lands in no column, so the row
 * adds nothing to the gradient, and its Q taken is NaN, which the two sums of stats_out then carry (tma_policy_evaluate_actions' rule).
 * Two launches; both forwards, the loss and the backward inside the first.  No float atomics: a gradient element is summed over the rows of a tile in
 * row order, over a workgroup's tiles in order, over the workgroups (at most 64: then they stride) in order -- equal inputs give equal bits.
 * `workspace`: tma_dqn_workspace_bytes(d, n) bytes of device memory, bounded whatever n (64 x the pi segment + 64 x 24 bytes at the most; 0 + message
 * for refused dims / n < 1).  Refused: NULL d / params / target_params / any input / grad_out, n < 1, a workspace that is NULL or too small. */
int64_t tma_dqn_workspace_bytes(const tma_policy_dims *d, int64_t n);
int tma_dqn_td_grad(const float *params, const float *target_params, const tma_policy_dims *d, const float *obs, const int32_t *actions,
                    const float *next_obs, const float *dones, const float *rewards, const float *discounts, int64_t n, float *grad_out,
                    double *stats_out, float *q_out, void *workspace, int64_t workspace_bytes, void *stream);
/* SB3's polyak_update over the trainable vector, element-wise in f32: target = tau * params + (1 - tau) * target (two products and a sum, nothing
 * fused); tau == 1 is a pure copy with the source's bits.  Then tma_policy_sync(target_params): the derived copies the tma_policy_* kernels read
 * from the target buffer (the DQN kernels read none of them).  Refused: NULL buffers, params == target_params, tau outside (0, 1] or NaN. */
int tma_dqn_target_update(const float *params, float *target_params, const tma_policy_dims *d, double tau, void *stream);
typedef struct {
    int64_t total_timesteps;        /* SB3's _total_timesteps: the denominator of the exploration schedule */
    int64_t learning_starts;
    int64_t batch_size;
    int64_t target_update_interval; /* in env steps: the target update runs when n_calls % max(target_update_interval / n_envs, 1) == 0 */
    int train_freq;                 /* vector steps collected per iteration */
    int gradient_steps;             /* optimizer steps per iteration; -1: train_freq */
    int n_step;                     /* tma_replay_sample's n_step */
    double tau, gamma;
    double exploration_fraction, exploration_initial_eps, exploration_final_eps;
    double learning_rate, max_grad_norm;
    uint32_t rng_seed;              /* tma_dqn_act's rng_seed */
    uint32_t sample_seed;           /* tma_replay_sample's seed */
    uint32_t env_offset;
} tma_dqn_hparams;
/* Device memory the native loop works in, all caller-owned.  N = the replay view's n_envs, D = obs_dim, B = batch_size. */
typedef struct {
    float *last_obs;      /* [N][D] in/out: the observation the next action is chosen from (ReplayBuffer.last_obs) */
    int32_t *actions;     /* [N] */
    float *step_obs;      /* [N][D] */
    float *rewards;       /* [N] */
    uint8_t *term, *trunc; /* [N] */
    float *term_obs;      /* [N][D] */
    float *s_obs;         /* [B][D]  the sampled batch */
    int32_t *s_actions;   /* [B] */
    float *s_next_obs;    /* [B][D] */
    float *s_dones, *s_rewards, *s_discounts; /* [B] */
    float *grad, *exp_avg, *exp_avg_sq; /* [n_trainable] */
    double *stats;        /* [3] tma_dqn_td_grad's stats_out of the last optimizer step; may be NULL */
    void *td_workspace;   /* tma_dqn_workspace_bytes(d, B) */
    int64_t td_workspace_bytes;
    void *opt_workspace;  /* tma_ppo_workspace_bytes(d): tma_ppo_adam_step_local's */
} tma_dqn_buffers;
/* Host counters, in/out: every decision of the loop is host arithmetic on them. */
typedef struct {
    int64_t num_timesteps; /* env steps taken (SB3's num_timesteps) */
    int64_t n_calls;       /* vector steps taken (SB3's _n_calls) */
    int64_t pos;           /* the ring row the next vector step is written to */
    int32_t full;          /* the ring has wrapped */
    uint32_t draw;         /* tma_replay_sample's draw counter of the next batch */
    uint32_t collect_step; /* tma_dqn_act's rng_step of the next vector step */
    int64_t adam_step;     /* optimizer steps taken: the next one is Adam step adam_step + 1 */
    int64_t n_updates;     /* SB3's _n_updates */
} tma_dqn_counters;
/* The exploration rate of the vector step taken at `num_timesteps` (host arithmetic, no GPU): 1 below learning_starts (SB3's uniform warm-up), else
 * SB3's get_linear_fn(initial, final, fraction) at progress_remaining = 1 - num_timesteps / total_timesteps, taken BEFORE the step. */
double tma_dqn_epsilon(const tma_dqn_hparams *hp, int64_t num_timesteps);
/* n_iters iterations of SB3's DQN.learn in one call, on the caller's stream, with no device -> host read and no synchronisation.  An iteration:
 * train_freq vector steps of  tma_dqn_act(last_obs, eps = tma_dqn_epsilon(hp, num_timesteps), rng_step = collect_step) -> tma_env_step (one step,
 * with term_obs) -> tma_replay_add(pos);  then collect_step += 1, pos advances (wraps, sets full), num_timesteps += N, n_calls += 1, and
 * tma_dqn_target_update(tau) where n_calls % max(target_update_interval / N, 1) == 0.  Then, if num_timesteps > learning_starts, gradient_steps times:
 * tma_replay_sample(size, newest from pos / full; draw) -> tma_dqn_td_grad -> tma_ppo_adam_step_local(step adam_step + 1, beta (0.9, 0.999),
 * eps 1e-8 -- torch Adam's default, which SB3's DQN uses --, max_grad_norm, last_count 0: the norm is taken from the gradient itself);  draw,
 * adam_step and n_updates advance.  The same launches in the same order as the calls issued one by one, hence the same bits.  `params` must be
 * synced on entry and is on return.  Refused before any HIP call: NULL arguments or buffers, bad dims, n_iters < 1, train_freq / batch_size /
 * target_update_interval < 1, gradient_steps 0 or below -1, exploration_fraction outside (0, 1], a replay view that is Box or of another obs_dim,
 * counters out of range.  The env handle, tau, n_step and the sample geometry are checked by the calls they go to. */
int tma_dqn_iterations_local(tma_env *env, float *params, float *target_params, const tma_policy_dims *d, const tma_replay *rb, const tma_dqn_buffers *b,
                             const tma_dqn_hparams *hp, tma_dqn_counters *c, int n_iters, void *stream);

/* ---- SAC (ABI 226): SB3's SAC (3P: stable_baselines3/sac/sac.py, SquashedDiagGaussianDistribution; the reference's off-policy choice for its Box
 *      tasks, backend/mlagents/training.py:392-403) -- csrc/tma_sac.hip, DESIGN.md section 18.
 * Shapes: hidden 64 / 128 / 256, 1 <= act_dim <= 8 (mu and log_std share one 16-column head tile), obs_dim + act_dim <= 128 (the critic's input
 * tile), f32, activation ReLU (SB3's SAC default) or tanh, exactly two critics.  Everything else is refused with TMA_ERR_INVALID and a message
 * before any HIP call, as are the NULLs and ranges each entry lists. */
typedef struct tma_sac_dims {
    int obs_dim, act_dim, hidden;
    int activation; /* TMA_ACT_TANH | TMA_ACT_RELU */
    int device;     /* HIP device ordinal, or -1: the current device */
} tma_sac_dims;
/* Float offsets into the flat [in][out] buffers, in SB3's tensor order.  Actor (n_actor floats): W1[D][H] b1 W2[H][H] b2 Wmu[H][A] bmu Wls[H][A]
 * bls = actor.latent_pi.{0,2}, actor.mu, actor.log_std.  Critic (n_critic = 2 n_q floats): qf0 then qf1 (at n_q), each W1[D+A][H] b1 W2[H][H] b2
 * W3[H][1] b3 with the observation rows of W1 first, then the action rows (SB3 concatenates obs | action); the q_* offsets are those inside ONE
 * critic.  The critic target is a second buffer of the critic layout.  There are no derived copies: nothing needs a sync after a write. */
typedef struct tma_sac_offsets {
    int a_W1, a_b1, a_W2, a_b2, a_Wmu, a_bmu, a_Wls, a_bls, n_actor;
    int q_W1, q_b1, q_W2, q_b2, q_W3, q_b3, n_q, n_critic;
} tma_sac_offsets;
int tma_sac_param_offsets(const tma_sac_dims *d, tma_sac_offsets *out);
/* The arithmetic of one row, with noise z f32[A]:  ls = clamp(log_std_head, -20, 2);  u = mu + exp(ls) z;  a = tanh(u);
 *   logp = sum_j (-z_j^2 / 2 - ls_j - log sqrt(2 pi)) - sum_j log(1 - a_j^2 + 1e-6)
 * with expf / logf / tanhf (not the fast intrinsics).  Noise: every noise-consuming entry takes noise_in f32[n][A] (may be NULL) and noise_out
 * (may be NULL).  With noise_in NULL, z of (row, column) is a Box-Muller pair of mix32 hashes of (seed ^ stream key, row id, draw), the stream key
 * being distinct for tma_sac_act (collect), tma_sac_critic_grad (next action) and tma_sac_actor_grad (pi action); feeding a call's noise_out back
 * as noise_in gives equal bits everywhere.  head_out (may be NULL): f32[n][2 A], the actor's mu then its log_std BEFORE the clamp -- one device
 * function in all three entries, so a row has the same bits in all three whatever the batch it came in. */
enum { TMA_SAC_SAMPLE = 0, TMA_SAC_DETERMINISTIC = 1, TMA_SAC_UNIFORM = 2 };
/* Actor forward plus squash in ONE launch.  mode SAMPLE: the row id of the hash is row_offset + row;  DETERMINISTIC: z = 0, a = tanh(mu) (noise_in
 * must be NULL; noise_out receives zeros);  UNIFORM: SB3's warm-up below learning_starts, a = 2 u01(mix32) - 1 in [-1, 1) per element without
 * reading the net (actor / obs may be NULL; noise_in, logp_out, noise_out, head_out must be).  actions_out f32[n][A]; logp_out f32[n] or NULL.
 * A workgroup of four waves per 16-row tile; the grid is capped and strides.  Refused: NULL d / actions_out, NULL actor / obs outside UNIFORM,
 * n < 1, an unknown mode. */
int tma_sac_act(const float *actor, const tma_sac_dims *d, const float *obs, int64_t n, int mode, uint32_t seed, uint32_t draw, uint32_t row_offset,
                const float *noise_in, float *actions_out, float *logp_out, float *noise_out, float *head_out, void *stream);
/* Bytes of device workspace either gradient call needs for n rows: at most 64 x (the wider of the critic pair and the actor) floats + 64 x 32
 * bytes, bounded whatever n (0 + message for refused dims / n < 1). */
int64_t tma_sac_workspace_bytes(const tma_sac_dims *d, int64_t n);
/* The critic side of SAC.train for one batch (what tma_replay_sample writes: obs f32[n][D], actions f32[n][A], next_obs f32[n][D], dones,
 * rewards, discounts f32[n]), with alpha = exp(log_ent_coef[0]) read from the device:
 *   a', logp' = the actor on next_obs (row id = row);   y = rewards + (1 - dones) * discounts * (min(Qt0, Qt1)(next_obs, a') - alpha logp')
 *   loss = 1/2 sum_i mean((Q_i(obs, actions) - y)^2)   (no gradient through y)
 * grad_out[n_critic] is OVERWRITTEN with its gradient.  stats_out (device, may be NULL): four float64 -- the sum over rows of
 * 1/2 ((Q0 - y)^2 + (Q1 - y)^2), sum Q0, sum Q1, n -- so critic_loss = stats[0] / stats[3].  q_out f32[n][2], target_out f32[n] (= y): optional.
 * Two launches (tile pass, slab fold).  No float atomics: a gradient element is summed over the rows of a tile in row order, over a workgroup's
 * tiles in order, over the workgroups (at most 64: then they stride) in order -- equal inputs give equal bits.
 * Refused: NULL d / any parameter buffer / any input / grad_out, n < 1, a workspace that is NULL or below tma_sac_workspace_bytes(d, n). */
int tma_sac_critic_grad(const float *actor, const float *critic, const float *critic_target, const float *log_ent_coef, const tma_sac_dims *d, const float *obs,
                        const float *actions, const float *next_obs, const float *dones, const float *rewards, const float *discounts, int64_t n, uint32_t seed,
                        uint32_t draw, const float *noise_in, float *grad_out, double *stats_out, float *q_out, float *target_out, float *noise_out,
                        float *head_out, void *workspace, int64_t workspace_bytes, void *stream);
/* The actor side:  a_pi, logp_pi = the actor on obs;  loss = mean(alpha logp_pi - min(Q0, Q1)(obs, a_pi)), on a tie qf0 carries the gradient.  The
 * backward goes through the winning critic's input gradient to the action rows only (no critic weight gradient is formed), then through the
 * squash and logp (the clamp passes the gradient where -20 <= log_std_head <= 2, torch's rule) into the actor.  grad_out[n_actor] is OVERWRITTEN.
 * stats_out (may be NULL): three float64 -- sum of (alpha logp_pi - min Q), sum of logp_pi, n.  actions_out f32[n][A], logp_out f32[n]: optional.
 * Launches, order of sums, workspace and refusals as tma_sac_critic_grad. */
int tma_sac_actor_grad(const float *actor, const float *critic, const float *log_ent_coef, const tma_sac_dims *d, const float *obs, int64_t n, uint32_t seed,
                       uint32_t draw, const float *noise_in, float *grad_out, double *stats_out, float *actions_out, float *logp_out, float *noise_out,
                       float *head_out, void *workspace, int64_t workspace_bytes, void *stream);
/* ent_coef="auto":  grad_out[0] = d/d log_ent_coef of -(log_ent_coef * (logp_pi + target_entropy)).mean() = -(stats[1] / stats[2] +
 * target_entropy), the mean taken in float64 from tma_sac_actor_grad's stats_out, rounded once to f32.  One launch of one thread. */
int tma_sac_ent_coef_grad(const double *actor_stats, double target_entropy, float *grad_out, void *stream);
/* torch.optim.Adam (no weight decay, no amsgrad, no clipping) on a flat f32 vector of n >= 1 elements, element-wise with the IEEE square root and
 * division:  m += (g - m)(1 - beta1);  v = v beta2 + g^2 (1 - beta2);  p -= (lr / (1 - beta1^step)) * (m / (sqrt(v) / sqrt(1 - beta2^step) + eps)),
 * the two bias corrections worked out on the host in double.  Steps the actor, the critic pair and the single log_ent_coef; there are no derived
 * copies to refresh.  Refused: NULL buffers, n < 1, step < 1, lr / eps below 0 or NaN, a beta outside [0, 1). */
int tma_adam_step_flat(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, double lr, double beta1, double beta2,
                       double eps, void *stream);
/* SB3's polyak_update on a flat range with tma_dqn_target_update's arithmetic: target = tau * params + (1 - tau) * target in f32 (two rounded
 * products and a sum, nothing fused); tau == 1 copies bits.  Refused: NULL buffers, n < 1, tau outside (0, 1] or NaN, params == target. */
int tma_polyak_update(const float *params, float *target, int64_t n, double tau, void *stream);
typedef struct {
    int64_t learning_starts;
    int64_t batch_size;
    int64_t target_update_interval; /* in optimizer steps: the polyak update follows the step taken at n_updates % interval == 0 */
    int train_freq;                 /* vector steps collected per iteration */
    int gradient_steps;             /* optimizer steps per iteration; -1: train_freq, one per VECTOR step collected (SB3: train_freq * n_envs) */
    int n_step;                     /* tma_replay_sample's n_step */
    int auto_ent_coef;              /* 1: ent_coef="auto" (the log_ent_coef step runs); 0: a fixed alpha */
    double tau, gamma, learning_rate, target_entropy;
    uint32_t rng_seed;              /* the noise seed of the three streams */
    uint32_t sample_seed;           /* tma_replay_sample's seed */
    uint32_t env_offset;            /* tma_sac_act's row_offset */
} tma_sac_hparams;
/* Device memory the native loop works in, all caller-owned.  N = the replay view's n_envs, D = obs_dim, A = act_dim, B = batch_size. */
typedef struct {
    float *last_obs;      /* [N][D] in/out: the observation the next action is chosen from */
    float *actions;       /* [N][A] */
    float *step_obs;      /* [N][D] */
    float *rewards;       /* [N] */
    uint8_t *term, *trunc; /* [N] */
    float *term_obs;      /* [N][D] */
    float *s_obs;         /* [B][D]  the sampled batch */
    float *s_actions;     /* [B][A] */
    float *s_next_obs;    /* [B][D] */
    float *s_dones, *s_rewards, *s_discounts; /* [B] */
    float *actor_grad, *actor_exp_avg, *actor_exp_avg_sq;    /* [n_actor] */
    float *critic_grad, *critic_exp_avg, *critic_exp_avg_sq; /* [n_critic] */
    float *ent_grad, *ent_exp_avg, *ent_exp_avg_sq;          /* [1] */
    double *critic_stats; /* [4] tma_sac_critic_grad's stats_out of the last optimizer step */
    double *actor_stats;  /* [3] tma_sac_actor_grad's */
    void *workspace;      /* tma_sac_workspace_bytes(d, B) */
    int64_t workspace_bytes;
} tma_sac_buffers;
/* Host counters, in/out: every decision of the loop is host arithmetic on them. */
typedef struct {
    int64_t num_timesteps; /* env steps taken */
    int64_t n_calls;       /* vector steps taken */
    int64_t pos;           /* the ring row the next vector step is written to */
    int32_t full;          /* the ring has wrapped */
    uint32_t draw;         /* tma_replay_sample's draw counter of the next batch, and the draw of its two noise streams */
    uint32_t collect_step; /* tma_sac_act's draw of the next vector step */
    int64_t adam_step;     /* optimizer steps taken: the next one is Adam step adam_step + 1 of all three optimizers */
    int64_t n_updates;     /* SB3's _n_updates */
} tma_sac_counters;
/* n_iters iterations of SB3's SAC.learn in one call, on the caller's stream, with no device -> host read and no synchronisation.  An iteration:
 * train_freq vector steps of  tma_sac_act(last_obs; UNIFORM while num_timesteps < learning_starts, else SAMPLE; draw = collect_step, row_offset =
 * env_offset) -> tma_env_step (one step, f32 actions, with term_obs) -> tma_replay_add(pos);  then collect_step += 1, pos advances (wraps, sets
 * full), num_timesteps += N, n_calls += 1.  Then, if num_timesteps > learning_starts, gradient_steps times:  tma_replay_sample(size, newest from
 * pos / full; draw) -> tma_sac_critic_grad(draw) -> tma_adam_step_flat(critic) -> tma_sac_actor_grad(draw; the critics AFTER their step, as SB3)
 * -> tma_adam_step_flat(actor) -> [auto_ent_coef: tma_sac_ent_coef_grad -> tma_adam_step_flat(log_ent_coef); both gradient kernels have read
 * the pre-step alpha by then] -> tma_polyak_update(critic -> critic_target, tau) where n_updates % target_update_interval == 0;  Adam with beta
 * (0.9, 0.999), eps 1e-8, step adam_step + 1;  then draw, adam_step and n_updates advance.  The same launches in the same order as the calls
 * issued one by one, hence the same bits.  Refused before any HIP call: NULL arguments or buffers, bad dims, n_iters < 1, train_freq /
 * batch_size / target_update_interval < 1, gradient_steps 0 or below -1, a replay view that is Discrete or of other dims, counters out of range. */
int tma_sac_iterations_local(tma_env *env, float *actor, float *critic, float *critic_target, float *log_ent_coef, const tma_sac_dims *d, const tma_replay *rb,
                             const tma_sac_buffers *b, const tma_sac_hparams *hp, tma_sac_counters *c, int n_iters, void *stream);

/* ---- TD3 (ABI 227): SB3's TD3 (3P: stable_baselines3/td3/td3.py; the reference's fifth algorithm, with SAC's value table,
 *      backend/mlagents/training.py:31-37, 392-403) -- csrc/tma_td3.hip, DESIGN.md section 19.
 * Shapes: tma_sac_dims and its contract (hidden 64 / 128 / 256, 1 <= act_dim <= 8, obs_dim + act_dim <= 128, f32, ReLU -- SB3's TD3 default -- or
 * tanh, exactly two critics), refused the same way.  Four flat [in][out] buffers in SB3's tensor order: the actor (n_actor floats) W1[D][H] b1
 * W2[H][H] b2 Wmu[H][A] bmu = actor.mu.{0,2,4}; the actor target, a second buffer of that layout; the critic pair and the critic target in SAC's
 * critic layout exactly (the q_* offsets equal tma_sac_param_offsets').  No derived copies. */
typedef struct tma_td3_offsets {
    int a_W1, a_b1, a_W2, a_b2, a_Wmu, a_bmu, n_actor;
    int q_W1, q_b1, q_W2, q_b2, q_W3, q_b3, n_q, n_critic;
} tma_td3_offsets;
int tma_td3_param_offsets(const tma_sac_dims *d, tma_td3_offsets *out);
/* SB3's NormalActionNoise per action column: noise_j = mean[j] + sigma[j] z_j.  Read on the host at the call and handed to the kernel by value;
 * columns at and behind act_dim are ignored. */
typedef struct tma_td3_noise {
    float mean[8], sigma[8];
} tma_td3_noise;
enum { TMA_TD3_DETERMINISTIC = 0, TMA_TD3_NOISY = 1, TMA_TD3_UNIFORM = 2 };
/* Actor forward and tanh in ONE launch: mu = the actor on obs, a = tanhf(mu).  mode DETERMINISTIC: a alone (noise_in must be NULL; noise_out
 * receives zeros; action_noise is ignored);  NOISY: a = clamp(tanhf(mu) + (mean_j + sigma_j z), -1, 1), SB3's action noise on the squashed action
 * -- z f32[n][A] from noise_in, or with noise_in NULL a Box-Muller pair of mix32 hashes of (seed ^ the collect stream key, row_offset + row,
 * draw), tma_sac_act's generator under a key of its own; action_noise must not be NULL, its sigmas at least 0;  UNIFORM: SB3's warm-up below
 * learning_starts with tma_sac_act's arithmetic and bits, the net is not read (actor / obs / action_noise may be NULL; noise_in, noise_out,
 * head_out must be).  actions_out f32[n][A];  noise_out f32[n][A] (z) and head_out f32[n][A] (mu BEFORE the tanh) may be NULL.  The actor
 * forward is one device function in all three TD3 entries: a row's mu has the same bits in each, whatever the batch it came in.  A workgroup of
 * four waves per 16-row tile; the grid is capped and strides.  Refused: NULL d / actions_out, NULL actor / obs outside UNIFORM, n < 1, an unknown
 * mode, NOISY without action_noise or with a negative / NaN sigma or a NaN mean. */
int tma_td3_act(const float *actor, const tma_sac_dims *d, const float *obs, int64_t n, int mode, const tma_td3_noise *action_noise, uint32_t seed,
                uint32_t draw, uint32_t row_offset, const float *noise_in, float *actions_out, float *noise_out, float *head_out, void *stream);
/* Bytes of device workspace either gradient call needs for n rows: at most 64 x (the wider of the critic pair and the actor) floats + 64 x 32
 * bytes, bounded whatever n (0 + message for refused dims / n < 1). */
int64_t tma_td3_workspace_bytes(const tma_sac_dims *d, int64_t n);
/* The critic side of TD3.train for one batch (what tma_replay_sample writes), no gradient through y:
 *   eps = clamp(target_policy_noise z, -target_noise_clip, +target_noise_clip);   a' = clamp(tanhf(mu_target(next_obs)) + eps, -1, 1)
 *   y = rewards + (1 - dones) * discounts * min(Qt0, Qt1)(next_obs, a');          loss = sum_i mean((Q_i(obs, actions) - y)^2)
 * SB3's sum(F.mse_loss(...)): the cotangent of Q_i is 2 (Q_i - y) / n (SAC's carries a 1/2).  z f32[n][A] from noise_in, or with noise_in NULL
 * generated from (seed ^ the target stream key, row, draw) -- a key distinct from tma_td3_act's.  grad_out[n_critic] is OVERWRITTEN.  stats_out
 * (device, may be NULL): four float64 -- the sum over rows of (Q0 - y)^2 + (Q1 - y)^2, sum Q0, sum Q1, n -- so critic_loss = stats[0] /
 * stats[3].  Optional: q_out f32[n][2], target_out f32[n] (= y), noise_out f32[n][A] (z), head_out f32[n][A] (mu_target(next_obs)).  Two
 * launches (tile pass, slab fold).  No float atomics; order of sums as tma_sac_critic_grad.  Refused: NULL d / any parameter buffer / any input /
 * grad_out, n < 1, a negative or NaN target_policy_noise / target_noise_clip, a workspace that is NULL or below tma_td3_workspace_bytes(d, n). */
int tma_td3_critic_grad(const float *actor_target, const float *critic, const float *critic_target, const tma_sac_dims *d, const float *obs, const float *actions,
                        const float *next_obs, const float *dones, const float *rewards, const float *discounts, int64_t n, double target_policy_noise,
                        double target_noise_clip, uint32_t seed, uint32_t draw, const float *noise_in, float *grad_out, double *stats_out, float *q_out,
                        float *target_out, float *noise_out, float *head_out, void *workspace, int64_t workspace_bytes, void *stream);
/* The actor side:  loss = -mean(Q0(obs, tanhf(mu(obs)))).  Only qf0 (the front n_q floats of `critic`) is read: its forward, its input gradient
 * down to the action rows of its W1 (no critic weight gradient is formed), through the tanh, then the actor's backward.  grad_out[n_actor] is
 * OVERWRITTEN.  stats_out (may be NULL): two float64 -- the sum of -Q0, n.  Optional: actions_out f32[n][A], head_out f32[n][A] (mu).  Launches,
 * order of sums, workspace and refusals as tma_td3_critic_grad. */
int tma_td3_actor_grad(const float *actor, const float *critic, const tma_sac_dims *d, const float *obs, int64_t n, float *grad_out, double *stats_out,
                       float *actions_out, float *head_out, void *workspace, int64_t workspace_bytes, void *stream);
typedef struct {
    int64_t learning_starts;
    int64_t batch_size;
    int64_t policy_delay;     /* the actor step and both target updates follow the critic step where n_updates % policy_delay == 0 */
    int train_freq;           /* vector steps collected per iteration */
    int gradient_steps;       /* optimizer steps per iteration; -1: train_freq, one per VECTOR step collected */
    int n_step;               /* tma_replay_sample's n_step */
    int use_action_noise;     /* 1: collect in the NOISY mode with action_noise; 0: DETERMINISTIC */
    double tau, gamma, learning_rate, target_policy_noise, target_noise_clip;
    tma_td3_noise action_noise;
    uint32_t rng_seed;        /* the noise seed of both streams and of the warm-up */
    uint32_t sample_seed;     /* tma_replay_sample's seed */
    uint32_t env_offset;      /* tma_td3_act's row_offset */
} tma_td3_hparams;
/* Device memory the native loop works in, all caller-owned; the fields of tma_sac_buffers without the entropy coefficient's. */
typedef struct {
    float *last_obs;      /* [N][D] in/out */
    float *actions;       /* [N][A] */
    float *step_obs;      /* [N][D] */
    float *rewards;       /* [N] */
    uint8_t *term, *trunc; /* [N] */
    float *term_obs;      /* [N][D] */
    float *s_obs;         /* [B][D]  the sampled batch */
    float *s_actions;     /* [B][A] */
    float *s_next_obs;    /* [B][D] */
    float *s_dones, *s_rewards, *s_discounts; /* [B] */
    float *actor_grad, *actor_exp_avg, *actor_exp_avg_sq;    /* [n_actor] */
    float *critic_grad, *critic_exp_avg, *critic_exp_avg_sq; /* [n_critic] */
    double *critic_stats; /* [4] tma_td3_critic_grad's stats_out of the last optimizer step */
    double *actor_stats;  /* [2] tma_td3_actor_grad's, of the last actor step */
    void *workspace;      /* tma_td3_workspace_bytes(d, B) */
    int64_t workspace_bytes;
} tma_td3_buffers;
/* Host counters, in/out: every decision of the loop is host arithmetic on them. */
typedef struct {
    int64_t num_timesteps;    /* env steps taken */
    int64_t n_calls;          /* vector steps taken */
    int64_t pos;              /* the ring row the next vector step is written to */
    int32_t full;             /* the ring has wrapped */
    uint32_t draw;            /* tma_replay_sample's draw counter of the next batch, and the draw of its target noise */
    uint32_t collect_step;    /* tma_td3_act's draw of the next vector step */
    int64_t critic_adam_step; /* critic steps taken: the next one is Adam step critic_adam_step + 1 */
    int64_t actor_adam_step;  /* actor steps taken (one per policy_delay critic steps) */
    int64_t n_updates;        /* SB3's _n_updates */
} tma_td3_counters;
/* n_iters iterations of SB3's TD3.learn in one call, on the caller's stream, with no device -> host read and no synchronisation.  An iteration:
 * train_freq vector steps of  tma_td3_act(last_obs; UNIFORM while num_timesteps < learning_starts, else NOISY where use_action_noise, else
 * DETERMINISTIC; draw = collect_step, row_offset = env_offset) -> tma_env_step (one step, f32 actions, with term_obs) -> tma_replay_add(pos);
 * then collect_step += 1, pos advances (wraps, sets full), num_timesteps += N, n_calls += 1.  Then, if num_timesteps > learning_starts,
 * gradient_steps times:  n_updates += 1 -> tma_replay_sample(size, newest from pos / full; draw) -> tma_td3_critic_grad(actor_target; draw) ->
 * tma_adam_step_flat(critic, step critic_adam_step + 1) -> where n_updates % policy_delay == 0: tma_td3_actor_grad (the critics AFTER their
 * step, as SB3) -> tma_adam_step_flat(actor, step actor_adam_step + 1) -> tma_polyak_update(critic -> critic_target, tau) ->
 * tma_polyak_update(actor -> actor_target, tau).  Adam with beta (0.9, 0.999), eps 1e-8.  The same launches in the same order as the calls issued
 * one by one, hence the same bits.  Refused before any HIP call: NULL arguments or buffers, bad dims, n_iters < 1, train_freq / batch_size /
 * policy_delay < 1, gradient_steps 0 or below -1, a negative target_policy_noise / target_noise_clip, a replay view that is Discrete or of other
 * dims, counters out of range. */
int tma_td3_iterations_local(tma_env *env, float *actor, float *actor_target, float *critic, float *critic_target, const tma_sac_dims *d, const tma_replay *rb,
                             const tma_td3_buffers *b, const tma_td3_hparams *hp, tma_td3_counters *c, int n_iters, void *stream);

/* Profiling aid for bench.py's roofline object: when enabled, tma_ppo_minibatch_grad brackets its DOMINANT kernel (the persistent
 * forward+backward kernel; for two-pass shapes both passes; not the advantage pass, not the slab reduction) with HIP events recorded on
 * the stream it launches on; tma_debug_last_grad_kernel_us waits for the last bracketed launch and returns its duration. */
int tma_debug_time_grad_kernel(int enable);
/* Test aid: fills the LDS of every CU with `pattern` (0: quiet NaNs) so that a kernel reading LDS it never wrote shows it in its outputs. */
int tma_debug_poison_lds(unsigned pattern, void *stream);
int tma_debug_last_grad_kernel_us(float *us_out);
/* Test aid: which specialisation the calling thread's last call of each policy dispatcher chose -- the forward (tma_policy_act / _act_bootstrap /
 * _values / _bootstrap), the minibatch gradient (tma_ppo_minibatch_grad and the epoch loops built on it) and the optimizer step
 * (tma_ppo_adam_step / _local).  Recorded on the host where each dispatcher decides, before its launches, whether or not they succeed;
 * TMA_DISPATCH_NONE after a call that was refused before a specialisation was picked.  Any pointer may be NULL.  No GPU work. */
enum {
    TMA_DISPATCH_NONE = 0,
    /* forward: H = 64 fast path; column-parallel kernels by dtype x hidden width (NTW = H / 64) x head; generic LDS kernel by waves per block */
    TMA_DISPATCH_FWD_H64 = 1,
    TMA_DISPATCH_FWD_F32_NTW2_DISCRETE = 2, TMA_DISPATCH_FWD_F32_NTW3_DISCRETE = 3, TMA_DISPATCH_FWD_F32_NTW4_DISCRETE = 4,
    TMA_DISPATCH_FWD_F32_NTW2_BOX = 5, TMA_DISPATCH_FWD_F32_NTW3_BOX = 6, TMA_DISPATCH_FWD_F32_NTW4_BOX = 7,
    TMA_DISPATCH_FWD_BF16_NTW2_DISCRETE = 8, TMA_DISPATCH_FWD_BF16_NTW3_DISCRETE = 9, TMA_DISPATCH_FWD_BF16_NTW4_DISCRETE = 10,
    TMA_DISPATCH_FWD_BF16_NTW2_BOX = 11, TMA_DISPATCH_FWD_BF16_NTW3_BOX = 12, TMA_DISPATCH_FWD_BF16_NTW4_BOX = 13,
    TMA_DISPATCH_FWD_GENERIC_W4 = 14, TMA_DISPATCH_FWD_GENERIC_W2 = 15, TMA_DISPATCH_FWD_GENERIC_W1 = 16,
    /* gradient: H = 64 kernel (<= 2048 samples: one tile per wave; else the persistent eight-wave kernel); three-term bf16 split.  (34 was
     * TMA_DISPATCH_GRAD_BF16 up to ABI 215: the bf16 kernels have one id per leaf below) */
    TMA_DISPATCH_GRAD_H64_SMALL = 32, TMA_DISPATCH_GRAD_H64 = 33, TMA_DISPATCH_GRAD_BF16X3 = 35,
    /* f32 column-parallel, layer-1 k-tiles kt1 = 1 (D <= 16) / 2 (D <= 32): half (16-row) or full row groups, four or eight waves,
     * dW2 deferred to the follow-up reduction or accumulated in the slabs */
    TMA_DISPATCH_GRAD_F32_KT1_HALF_W4 = 36, TMA_DISPATCH_GRAD_F32_KT1_FULL_W4 = 37, TMA_DISPATCH_GRAD_F32_KT2_HALF_W4 = 38,
    TMA_DISPATCH_GRAD_F32_KT2_FULL_W4 = 39, TMA_DISPATCH_GRAD_F32_KT1_HALF_W8_DEFER = 40, TMA_DISPATCH_GRAD_F32_KT1_HALF_W8_SLAB = 41,
    TMA_DISPATCH_GRAD_F32_KT1_FULL_W8 = 42, TMA_DISPATCH_GRAD_F32_KT2_HALF_W8_DEFER = 43, TMA_DISPATCH_GRAD_F32_KT2_HALF_W8_SLAB = 44,
    TMA_DISPATCH_GRAD_F32_KT2_FULL_W8 = 45,
    /* kt1 = 7 (H = 256, 33..112 observations, <= 1024 samples): half groups, eight waves, dW2 deferred */
    TMA_DISPATCH_GRAD_F32_SMALL7 = 46,
    /* two passes (chain, then dW1) with 11 / 7 layer-1 k-tiles, dW1 from the cached dz1 operands or a recomputed chain; runtime width */
    TMA_DISPATCH_GRAD_F32_KT11_CACHED = 47, TMA_DISPATCH_GRAD_F32_KT11_RECOMPUTE = 48, TMA_DISPATCH_GRAD_F32_KT107_CACHED = 49,
    TMA_DISPATCH_GRAD_F32_KT107_RECOMPUTE = 50, TMA_DISPATCH_GRAD_F32_KT0 = 51,
    /* generic float-atomic kernel by waves per block */
    TMA_DISPATCH_GRAD_GENERIC_W4 = 52, TMA_DISPATCH_GRAD_GENERIC_W3 = 53, TMA_DISPATCH_GRAD_GENERIC_W2 = 54, TMA_DISPATCH_GRAD_GENERIC_W1 = 55,
    /* bf16 column-parallel (ABI 216; plan_grad_bf): dW1 in registers, one (D <= 16) / two (D <= 32) k-tiles, 32-row (MT2) or 64-row (MT4) groups,
     * _W8: eight waves (Discrete head, H = 256); two passes with 2 (33..64 observations) / 6 (161..192) / 4 (97..128, Box head, H = 256) layer-1
     * k-steps, dW1 from the cached dz1 images or a recomputed chain, _W8: eight waves (Box head, H = 256); any other width: runtime width */
    TMA_DISPATCH_GRAD_BF16_KT1_MT2 = 80, TMA_DISPATCH_GRAD_BF16_KT1_MT4 = 81, TMA_DISPATCH_GRAD_BF16_KT1_MT4_W8 = 82,
    TMA_DISPATCH_GRAD_BF16_KT2_MT2 = 83, TMA_DISPATCH_GRAD_BF16_KT2_MT4 = 84,
    TMA_DISPATCH_GRAD_BF16_KS2_CACHED = 85, TMA_DISPATCH_GRAD_BF16_KS2_RECOMPUTE = 86, TMA_DISPATCH_GRAD_BF16_KS6_CACHED = 87,
    TMA_DISPATCH_GRAD_BF16_KS6_RECOMPUTE = 88, TMA_DISPATCH_GRAD_BF16_KS6_W8_CACHED = 89, TMA_DISPATCH_GRAD_BF16_KS6_W8_RECOMPUTE = 90,
    TMA_DISPATCH_GRAD_BF16_KS4_W8_CACHED = 91, TMA_DISPATCH_GRAD_BF16_KS4_W8_RECOMPUTE = 92, TMA_DISPATCH_GRAD_BF16_RUNTIME = 93,
    /* optimizer: Adam + scatter into the derived copies (H = 64 fast path / column-parallel layouts); single-block kernel; multi-block kernel
     * + tma_policy_sync; the _local forms of the two scatters, which fold the norm partials the gradient's reduction left */
    TMA_DISPATCH_OPT_SCATTER_H64 = 64, TMA_DISPATCH_OPT_SCATTER_WIDE = 65, TMA_DISPATCH_OPT_SMALL = 66, TMA_DISPATCH_OPT_ADAM = 67,
    TMA_DISPATCH_OPT_LOCAL_SCATTER_H64 = 68, TMA_DISPATCH_OPT_LOCAL_SCATTER_WIDE = 69,
    /* flag on a forward or generic-gradient id: the grid is capped and the kernel loops over it */
    TMA_DISPATCH_GRID_CAPPED = 256
};
/* The optimizer ids of the RMSpropTFLike step (tma_rmsprop_step / _local, ABI 214): the same six kernel shapes, chosen by the same plan -- the
 * Adam id + 8.  (Not members of the enum above: that table is the one tests/test_policy_dispatch_gpu.py holds a float64 case for, id by id; these
 * have theirs in tests/test_a2c_gpu.py.)  tma_debug_plan_dispatch answers with the Adam ids for both optimizers. */
#define TMA_DISPATCH_OPT_RMSPROP_SCATTER_H64 72
#define TMA_DISPATCH_OPT_RMSPROP_SCATTER_WIDE 73
#define TMA_DISPATCH_OPT_RMSPROP_SMALL 74
#define TMA_DISPATCH_OPT_RMSPROP_STEP 75
#define TMA_DISPATCH_OPT_RMSPROP_LOCAL_SCATTER_H64 76
#define TMA_DISPATCH_OPT_RMSPROP_LOCAL_SCATTER_WIDE 77
int tma_debug_last_dispatch(int32_t *fwd_out, int32_t *grad_out, int32_t *opt_out);
/* Test aid (ABI 213): what those dispatchers WOULD choose, asked on the host alone -- no HIP call, so it answers on a machine without a GPU.  `which`
 * selects the dispatcher and says what `n` is: TMA_PLAN_FWD -- tma_policy_act on n rows; TMA_PLAN_GRAD -- tma_ppo_minibatch_grad on a minibatch
 * of n samples; TMA_PLAN_OPT -- tma_ppo_adam_step (n unused); TMA_PLAN_OPT_LOCAL -- tma_ppo_adam_step_local with last_count = n.  It validates
 * `d` as the real call does, runs the same pure plan function (csrc/tma_policy_plan.h) with the environment switches the real call would read,
 * and returns the real call's status and message where that would refuse the shape.  *id_out: the id tma_debug_last_dispatch reports after
 * the real call.  grid / block / LDS bytes: the forward kernel's; the gradient's dominant kernel (the first of the two launches of the
 * two-pass kernels; ABI 216: the bf16 kernels' too) -- but *lds_bytes_out = -1 where the family's own launcher picks that geometry (H = 64, three-term split): grid and
 * block are then the slab reduction's that follows; the optimizer kernel's that steps the parameters (LDS 0).  Any output pointer may be NULL. */
#define TMA_PLAN_FWD 0
#define TMA_PLAN_GRAD 1
#define TMA_PLAN_OPT 2
#define TMA_PLAN_OPT_LOCAL 3
int tma_debug_plan_dispatch(const tma_policy_dims *d, int which, int64_t n, int32_t *id_out, int64_t *grid_out, int32_t *block_out, int32_t *lds_bytes_out);
/* out8: sums since the last call of {policy_loss, value_sq_err, entropy, approx_kl, clipped, n_samples}, then the last
 * total grad norm and clip coefficient.  Synchronises `stream`. */
int tma_ppo_pop_stats(void *workspace, double *out8_host, void *stream);
/* The same in two phases, for a loop that must not wait for the update it has just queued: tma_ppo_stats_enqueue copies the raw slots into
 * `staging_host` (tma_ppo_stats_staging_bytes() bytes of host memory; pinned memory makes the copy asynchronous) and clears them, ordered
 * on `stream`, without waiting; after the caller has synchronised with that point of the stream tma_ppo_stats_fold(staging_host, out8)
 * returns what tma_ppo_pop_stats would have. */
int64_t tma_ppo_stats_staging_bytes(void);
int tma_ppo_stats_enqueue(void *workspace, void *staging_host, void *stream);
int tma_ppo_stats_fold(const void *staging_host, double *out8_host);

/* Clear the statistic slots ordered on `stream` without reading them (ABI 214): the next tma_ppo_stats_enqueue / tma_ppo_pop_stats then reports
 * the updates queued after this call alone. */
int tma_ppo_stats_clear(void *workspace, void *stream);

/* ---- native rollout loop: SB3 OnPolicyAlgorithm.collect_rollouts driven by model.learn()
 *      (backend/mlagents/training.py:166-170; SURVEY.md §3.1 loop A) without a host round-trip per step ---- */
typedef struct {
    float *obs;            /* [T+1][N][D]; slot t is the observation acted on at step t, slot T the final new_obs */
    void *actions;         /* [T][N] i32 or [T][N][A] f32 */
    float *rewards;        /* [T][N], timeout bootstrap already applied */
    float *values;         /* [T][N] */
    float *log_probs;      /* [T][N] */
    uint8_t *terminated;   /* [T][N] */
    uint8_t *truncated;    /* [T][N] */
    float *terminal_obs;   /* [K][N][D] scratch (K = terminal_obs_slots): slot (t mod K) holds step t's pre-reset observations */
    float *last_values;    /* [N] */
    int64_t N;
    int terminal_obs_slots; /* K >= 1 (0 is read as 1).  With K > 1 the non-fused path computes the timeout bootstrap
                               rewards[t] += gamma * V(terminal_obs[t]) of K consecutive steps in ONE launch over K*N rows
                               instead of one small launch per vector step */
} tma_rollout_buffers;
/* One launch advances every env by many vector steps ("fused chunk") for the shapes of six kernel families; every other shape runs policy
 * forward + env step launch by launch -- the same results bit for bit (tests/test_ppo_gpu.py::test_native_rollout_equals_stepwise_composition).
 * Which family runs a shape, its precedence, thresholds and switches: DESIGN.md 4.3 (csrc/tma_rollout_plan.h; tma_debug_plan_rollout answers it).
 * deterministic != 0: actions are the distribution's mode (first maximal logit / Gaussian mean) instead of samples -- what SB3's
 * evaluate_policy(deterministic=True) asks of the policy (backend/mlagents/training.py:177-184,240-247); evaluation.py runs whole evaluation
 * chunks through this entry point and reads the finished episodes from the env's episode log. */
int tma_rollout_collect(tma_env *env, const float *params, const tma_policy_dims *d, const tma_rollout_buffers *b, int t_begin, int t_end,
                        int T, uint32_t rng_seed, uint32_t rng_step0, uint32_t env_offset, double gamma, int compute_last_values,
                        int deterministic, void *stream);
/* Test aid (ABI 211): waves per 16-env tile of the 64-wide fused chunk kernel the calling thread's last tma_rollout_collect launched -- 8, 4
 * (TMA_ROLL4=1, and Glider always: its env step needs a four-wave workgroup's registers), 2 (TMA_ROLL2=1), 1 (16 384 envs and more: four tiles a workgroup, one wave each); 0 before the first such launch.  No GPU work. */
int tma_debug_last_rollout_waves(void);
/* GAE from done flags (episode_starts[t+1] == terminated[t] | truncated[t]): same arithmetic as tma_gae */
int tma_gae_flags(const float *rewards, const float *values, const uint8_t *terminated, const uint8_t *truncated,
                  const float *last_values, double gamma, double gae_lambda, int T, int64_t N, float *adv_out, float *ret_out,
                  void *stream);

/* ---- A2C (ABI 214): replaces the SB3 objects A2C("MlpPolicy", env, **kwargs) builds when backend/mlagents/training.py:150 is reached with
 *      `--algorithm a2c` (algorithm table training.py:31-37; _default_model_kwargs gives A2C only tensorboard_log and verbose, so SB3's defaults:
 *      net_arch [64, 64], n_steps 5, RMSpropTFLike(alpha 0.99, eps 1e-5), max_grad_norm 0.5).  Semantics: SB3 2.9. ----
 * clip_grad_norm_(max_grad_norm) + RMSpropTFLike.step() (+ refresh of the derived copies): the counterpart of tma_ppo_adam_step, on the same
 * kernel shapes (tma_debug_plan_dispatch(TMA_PLAN_OPT) names the shape; tma_debug_last_dispatch reports TMA_DISPATCH_OPT_RMSPROP_*).  With g the
 * gradient scaled by grad_scale and by the clip coefficient min(1, max_grad_norm / (norm + 1e-6)):
 *     square_avg = alpha * square_avg + (1 - alpha) * g * g          (the caller starts square_avg at ONES: the "TF-like" part)
 *     p          = p - lr * g / sqrt(square_avg + eps)               (eps INSIDE the root)
 * No weight decay, momentum or centering.  Per element in f32 with the IEEE square root and division; the norm is a fixed-order f64 sum, so the
 * step is bit-identical from run to run.  grad is zero afterwards.  lr, eps >= 0 and finite, alpha in [0, 1).  Null buffers, bad dims and bad
 * constants are refused (TMA_ERR_INVALID) before any HIP call. */
int tma_rmsprop_step(float *params, float *grad, float *square_avg, const tma_policy_dims *d, double lr, double alpha, double eps, double max_grad_norm,
                     double grad_scale, void *workspace, void *stream);
/* The counterpart of tma_ppo_adam_step_local: `grad` is exactly what the LAST gradient call on this workspace produced over last_count samples; the
 * norm partials are read where that gradient's reduction left them (where tma_debug_plan_dispatch(TMA_PLAN_OPT_LOCAL, last_count) says it did), else
 * this is tma_rmsprop_step(grad_scale = 1). */
int tma_rmsprop_step_local(float *params, float *grad, float *square_avg, const tma_policy_dims *d, double lr, double alpha, double eps, double max_grad_norm,
                           void *workspace, void *stream, int64_t last_count);
typedef struct {
    double ent_coef, vf_coef;
    int normalize_advantage;
} tma_a2c_hparams;
/* One A2C.train(): the gradient of  -(adv * log_prob).mean() + ent_coef * -(entropy.mean()) + vf_coef * mse(returns, values)  over all T * N samples
 * of the rollout view as ONE minibatch, then tma_rmsprop_step_local, issued natively.  The gradient launches are tma_ppo_minibatch_grad's with a
 * clip range that never clips: the surrogate is then -adv * ratio, whose gradient at ratio = 1 is the one above.
 * CONTRACT: rb->log_probs are the log-probabilities of rb->actions under `params` -- what the rollout wrote.  A2C updates once, right after the
 * rollout, so this holds by construction; a caller that fills the plane itself uses tma_policy_evaluate_actions on the same parameters.
 * Batches of up to 256 samples that land on the generic gradient kernel (float atomics) run it as one wave per net, its tiles in turn, so
 * that the update is bit-identical from run to run at A2C's batch sizes; the H = 64 and column-parallel kernels end in a fixed-order reduction anyway.
 * Statistics (tma_ppo_stats_enqueue + tma_a2c_stats_fold): policy_loss is SB3's -(adv * log_prob).mean() (a reduction kernel of its own over the
 * two planes), value_loss and entropy as PPO's; approx_kl and clip_fraction are not reported.  grad must be zero on entry and is zero on return. */
int tma_a2c_update_local(float *params, const tma_policy_dims *d, const tma_rollout *rb, const tma_a2c_hparams *hp, float *grad, float *square_avg, double lr,
                         double alpha, double eps, double max_grad_norm, void *workspace, void *stream);
/* Its gradient half alone (the gradient launches and the policy-loss reduction; grad accumulates): what A2C(use_rms_prop=False) puts in front of
 * tma_ppo_adam_step_local, as SB3 steps that variant with Adam. */
int tma_a2c_grad(const float *params, const tma_policy_dims *d, const tma_rollout *rb, const tma_a2c_hparams *hp, float *grad, void *workspace, void *stream);
/* n_iterations whole A2C iterations in one call, with no host-language round trip between them (at the reference's 8 envs x 5 steps an iteration
 * is 40 samples: the path is launch- and host-bound).  Each iteration, in order: [copy of observation slot T into slot 0 -- from the second
 * iteration on, and in front of the first when carry_first != 0], tma_rollout_collect over [0, T) with rng_step0 = (rollout_counter0 + i) * T (the
 * sampling counters of PPO.collect_rollouts), tma_gae_flags, tma_ppo_pack_samples where the shape has records and `packed` is not NULL,
 * tma_a2c_update_local.  The same launches in the same order as the per-iteration calls, hence the same bits.  advantages / returns: [T][N] planes
 * the GAE writes; the statistic slots are cleared in front of the LAST iteration's update, so what a caller reads afterwards is that update's
 * (SB3 logs the last update's losses).  `env` is a device handle: null arguments are refused before any HIP call, everything else needs the GPU. */
int tma_a2c_iterations_local(tma_env *env, float *params, const tma_policy_dims *d, const tma_rollout_buffers *buffers, float *advantages, float *returns,
                             float *packed, int T, uint32_t rng_seed, uint32_t rollout_counter0, uint32_t env_offset, double gamma, double gae_lambda,
                             int carry_first, int n_iterations, const tma_a2c_hparams *hp, float *grad, float *square_avg, double lr, double alpha, double eps,
                             double max_grad_norm, void *workspace, void *stream);
/* tma_ppo_stats_fold for an A2C update: out8 = {sum of -(adv * log_prob), value_sq_err, entropy, 0, 0, n_samples, grad norm, clip coefficient} */
int tma_a2c_stats_fold(const void *staging_host, double *out8_host);

/* ---- VecNormalize (ABI 217): SB3's VecNormalize wrapper -- running mean / variance of the observations and of the per-env discounted
 *      returns, normalisation and clipping of observations and rewards -- on the device.  SB3 users put it around the vector env for tasks with
 *      unbounded observations and wide return ranges; the reference's own runs do not use it, so nothing selects it unless the caller does.
 * The handle owns, in device memory, all float64: obs mean[D], var[D], count; return mean, var, count; returns[N]; and float32 copies of the last
 * step's raw observations [N][D] and rewards [N].  Device memory is allocated on the handle's first use, so tma_vecnorm_create and every argument
 * check below answer without a GPU; that first use -- the first reset, step, rollout or statistics call on the handle -- allocates, fills the
 * buffers with synchronous copies and drains the device ONCE (hipDeviceSynchronize), later calls wait for nothing.  Initial statistics are RunningMeanStd(epsilon = 1e-4)'s: mean 0, var 1, count 1e-4.
 * A batch's moments are float64, two-pass (mean, then the sum of squared distances from it; never E[x^2] - E[x]^2), summed in an order that
 * (N, D) alone fixes -- no float atomics, run-to-run bit-identical -- and merged into the running ones by exactly
 *     delta = bm - mean;  tot = count + n;  mean' = mean + delta * n / tot;
 *     M2 = var * count + bv * n + delta * delta * count * n / tot;  var' = M2 / tot;  count' = tot
 * normalize_obs(o) = float(clip((double(o) - mean) / sqrt(var + epsilon), -clip_obs, clip_obs)), normalize_reward(r) =
 * float(clip(double(r) / sqrt(ret_var + epsilon), -clip_reward, clip_reward)): IEEE subtract, square root and divide in float64.
 * Up to TMA_VECNORM_ONE_LAUNCH_MAX envs a training step is ONE launch of one workgroup; beyond it two (per-workgroup partial moments, then a
 * fixed-order fold every workgroup repeats in front of its own rows).  All calls on one handle must be ordered on one stream.
 * Refused with TMA_ERR_INVALID before any HIP call: NULL handles or planes, D <= 0 or > TMA_VECNORM_MAX_DIM, N <= 0, clips or epsilon that are
 * not positive, gamma outside [0, 1], a row count or observation width that differs from the handle's. */
#define TMA_VECNORM_ONE_LAUNCH_MAX 256
#define TMA_VECNORM_MAX_DIM 1024
typedef struct tma_vecnorm tma_vecnorm;
int tma_vecnorm_create(int D, int64_t N, int norm_obs, int norm_reward, double clip_obs, double clip_reward, double gamma, double epsilon, int device,
                       tma_vecnorm **out);
int tma_vecnorm_destroy(tma_vecnorm *h);
/* norm_obs / norm_reward may change after construction (SB3 exposes them as attributes) */
int tma_vecnorm_set_flags(tma_vecnorm *h, int norm_obs, int norm_reward);
/* VecNormalize.reset(): returns = 0; training && norm_obs: the observation statistics take obs[n][D]; obs is normalised in place.  n == N. */
int tma_vecnorm_reset(tma_vecnorm *h, float *obs, int64_t n, int training, void *stream);
/* VecNormalize.step_wait() on the outputs of one vector step, in place, in SB3's order: (1) training && norm_obs: the observation statistics take
 * obs; (2) obs is normalised; (3) training: returns = returns * gamma + rewards and the return statistics take returns (whether or not norm_reward
 * is set); (4) rewards are normalised; (5) where terminated | truncated, terminal_obs (may be NULL) is normalised with the statistics of (1) --
 * terminal observations never enter them; (6) returns = 0 where terminated | truncated.  The raw obs and rewards are kept (tma_vecnorm_get_original). */
int tma_vecnorm_step(tma_vecnorm *h, float *obs, float *rewards, float *terminal_obs, const uint8_t *terminated, const uint8_t *truncated, int64_t n,
                     int training, void *stream);
/* stateless maps with the current statistics over any n rows; in and out are device memory and may be the same; identity where the flag is off */
int tma_vecnorm_normalize_obs(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream);
int tma_vecnorm_unnormalize_obs(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream);     /* float(double(o) * sqrt(var + eps) + mean) */
int tma_vecnorm_normalize_reward(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream);
int tma_vecnorm_unnormalize_reward(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream);  /* float(double(r) * sqrt(ret_var + eps)) */
/* statistics to / from HOST float64: obs_mean[D], obs_var[D], scalars4 = {obs count, return mean, return var, return count}.  Synchronise `stream`. */
int tma_vecnorm_get_stats(tma_vecnorm *h, double *obs_mean_host, double *obs_var_host, double *scalars4_host, void *stream);
int tma_vecnorm_set_stats(tma_vecnorm *h, const double *obs_mean_host, const double *obs_var_host, const double *scalars4_host, void *stream);
/* sync_envs_normalization: dst's statistics = src's, device to device, ordered on `stream` (same D) */
int tma_vecnorm_copy_stats(tma_vecnorm *dst, tma_vecnorm *src, void *stream);
/* the per-env discounted returns to HOST float64[N] (synchronises `stream`) */
int tma_vecnorm_get_returns(tma_vecnorm *h, double *returns_host, void *stream);
/* get_original_obs / get_original_reward: the raw values of the last reset / step into DEVICE memory [N][D] / [N]; either may be NULL */
int tma_vecnorm_get_original(tma_vecnorm *h, float *obs_out, float *rewards_out, void *stream);
/* tma_rollout_collect's per-step composition (policy forward, env step, timeout bootstrap; both its K == 1 form and its terminal-observation
 * window) with one tma_vecnorm_step behind every tma_env_step, BEFORE the bootstrap that reads that step's terminal_obs and rewards: SB3 adds
 * gamma * V(normalised terminal observation) to the normalised reward.  The buffers end up holding normalised observations and rewards.
 * b->obs slot t_begin must hold NORMALISED observations (tma_vecnorm_reset, or the previous call's last slot).  training = 0 freezes the
 * statistics (evaluation).
 * ABI 219: where tma_rollout_norm_plan answers with a fused value, and the env handle is reset, the VecNormalize step runs INSIDE the 8-env-tile
 * f32 fused chunk kernel of tma_rollout_collect -- one launch per chunk (bounded by tma_env_steps_until_refill and terminal_obs_slots) plus one
 * batched tma_policy_values and one tma_policy_bootstrap launch over the chunk's normalised rows -- with the running statistics in LDS for the
 * whole chunk.  It leaves, bit for bit, what the per-step composition leaves: buffers, statistics, returns, the raw copies.  Every other shape
 * runs launch by launch as before; TMA_NO_NORM_FUSED=1 (read once) keeps every shape there. */
int tma_rollout_collect_norm(tma_env *env, tma_vecnorm *vn, const float *params, const tma_policy_dims *d, const tma_rollout_buffers *b, int t_begin,
                             int t_end, int T, uint32_t rng_seed, uint32_t rng_step0, uint32_t env_offset, double gamma, int compute_last_values,
                             int deterministic, int training, void *stream);
/* Which path tma_rollout_collect_norm takes for (task, dims, N envs, training) (ABI 219; a host-only query, no HIP call).  Fused where
 * tma_rollout_collect would run its 8-env-tile f32 chunk kernel for the 256-wide policy -- hidden 256, f32 operands, obs_dim / act_dim the
 * task's; Discrete tasks, or Crawler / Ant with Box actions -- and, with training != 0, N <= 8: the vector is then one tile and a step's
 * moments one workgroup's work; with training == 0 rows are independent and N may reach the kernel's own cap (2048 Discrete, 4096 Box).
 * Everything else is PER_STEP.  Bad dims, N < 1 or an unknown task: -TMA_ERR_INVALID / -TMA_ERR_UNKNOWN_TASK. */
enum { TMA_ROLLOUT_NORM_PER_STEP = 0, TMA_ROLLOUT_NORM_FUSED_DISC_F32 = 1, TMA_ROLLOUT_NORM_FUSED_CONT_F32 = 2 };
int tma_rollout_norm_plan(int task, const tma_policy_dims *d, int64_t N, int training);
/* Test aid (ABI 219): the plan value the calling thread's last tma_rollout_collect_norm actually launched (PER_STEP also where a switch or an
 * env handle that is not reset kept it off the fused kernels). */
int tma_debug_last_rollout_norm_path(void);
/* The plan behind tma_rollout_collect / tma_rollout_collect_norm (ABI 223; host-only queries, no HIP call).
 * tma_debug_plan_rollout: what the driver would run for (task, dims, N envs, reset env handle or not, terminal_obs_slots, norm) under this
 * process's switches -- out6 = {family, waves per 16-env tile (H64 only, else 0), envs per tile or group (PER_STEP: 0), grid, block, LDS bytes of
 * the chunk kernel (PER_STEP launches none: 1, 64, 0)}.  norm: NONE for tma_rollout_collect, TRAINING / FROZEN for tma_rollout_collect_norm.
 * It refuses what the real calls refuse: NULL arguments, bad dims, an unknown task, N < 1.
 * tma_debug_last_rollout_plan: out3 = {family, waves, rows} of the calling thread's last tma_rollout_collect / tma_rollout_collect_norm. */
enum { TMA_ROLLOUT_FAMILY_PER_STEP = 0, TMA_ROLLOUT_FAMILY_H64 = 1, TMA_ROLLOUT_FAMILY_BF16_DISC = 2, TMA_ROLLOUT_FAMILY_BF16_BOX_TWO_NET = 3,
       TMA_ROLLOUT_FAMILY_BF16_BOX_PI = 4, TMA_ROLLOUT_FAMILY_F32_DISC = 5, TMA_ROLLOUT_FAMILY_F32_BOX = 6 };
enum { TMA_ROLLOUT_PLAN_NORM_NONE = 0, TMA_ROLLOUT_PLAN_NORM_TRAINING = 1, TMA_ROLLOUT_PLAN_NORM_FROZEN = 2 };
int tma_debug_plan_rollout(int task, const tma_policy_dims *d, int64_t N, int is_reset, int terminal_obs_slots, int norm, int32_t *out6);
int tma_debug_last_rollout_plan(int32_t *out3);

#ifdef __cplusplus
}
#endif
#endif
