// tma_dqn.hip -- SB3's DQN on the device (ABI 225): tma_dqn_act, tma_dqn_td_grad, tma_dqn_target_update, tma_dqn_iterations_local.
// The Q-network is the `pi.*` segment of a Discrete tma_policy_dims parameter buffer (features -> H -> H -> A, SB3's QNetwork); the `vf.*` segment
// is never read and its gradient is exact zeros.  The target net is a second buffer of the same layout, of which only the trainable [in][out]
// matrices are read.  f32 MFMA (v_mfma_f32_16x16x4_f32: bitwise a k-ordered fmaf chain), no float atomics, every sum in a fixed order.
//
// Unit of work: ONE workgroup of four waves owns a tile of 16 rows.  A hidden layer's H output columns are split over the waves (16 NT columns
// each, NT = H / 64), the tile's activations live in LDS, a barrier separates the layers; the head (one 16-column MFMA tile) is wave 0's.
// dqn_q_tile is the ONE forward: tma_dqn_act and both nets of tma_dqn_td_grad run it on the same thread layout, so a row's Q has the same bits
// in all three whatever the batch it came in.
//
// tma_dqn_act: one launch -- dqn_q_tile, then lane `row` of wave 0 applies tma_egreedy_actions' rule to its row of the Q tile in LDS.
// tma_dqn_td_grad: two launches.
//   (1) dqn_td_kernel: grid min(tiles, DQN_GRID_CAP), a block walks tiles b, b + grid, ...  Per tile: target forward on next_obs, online forward
//       on obs, lane `row` forms y, delta, the Huber value and the head cotangent; then dW3 / db3, dz2 (in place of h2), dW2 / db2, dz1 (in
//       place of h1), dW1 / db1.  A weight-gradient element is owned by one lane of one wave of the block, which stores it into the block's
//       slab at the block's first tile and adds to it (plain load-add-store, program order of one thread) at the later ones.
//   (2) dqn_reduce_kernel: grad[e] = slab_0[e] + slab_1[e] + ... in block order over the pi segment, exact zeros behind it; thread 0 folds the
//       blocks' (loss, Q taken, count) float64 partials in block order.
// Order of one gradient element's sum: rows in order inside a tile (the MFMA's k order), a block's tiles in order, blocks in order: it depends on
// (shape, n) alone, so equal inputs give equal bits.  The workspace is grid x (pi segment + 3 doubles), bounded by the grid cap whatever n.
// The layer functions, mlp_trunk_tile (the two hidden layers of dqn_q_tile), TileStats, TILE_DISPATCH, tile_set_device and the native loop's
// collect step and sample live in tma_dqn_tile.h, which tma_sac.hip and tma_td3.hip share; the target update runs tma_sac.hip's polyak kernel.
#include "tma_dqn_tile.h"

namespace tma {

constexpr int DQN_GRID_CAP = 64;   // workgroups of dqn_td_kernel at the most (= slabs in the workspace); more tiles are walked with this stride
constexpr int DQN_ACT_GRID_CAP = 1024;
constexpr uint32_t DQN_PICK_KEY = 0xE9517EEDu;  // tma_egreedy_actions' EGREEDY_PICK_KEY (tma_replay.hip): the same hash, the same actions

// THE forward: q[16][DQN_LDQ] (columns < A) = Q(X) of the pi segment of `p`; h1, h2 keep the hidden activations.  Every thread of the workgroup
// calls it (it holds barriers); X must be complete (a barrier behind its load); on return q, h1, h2 are visible to every thread.
template <int ACT, int NT>
__device__ __forceinline__ void dqn_q_tile(const float *__restrict__ p, const PLayout &L, const float *X, float *h1, float *h2, float *q, int lane, int wave) {
    constexpr int H = 64 * NT, LD = H + 2;
    mlp_trunk_tile<ACT, NT>(X, L.D, p, L.pW1t, L.pb1, L.pW2t, L.pb2, h1, h2, lane, wave);
    if (wave == 0) {
        f32x4 acc[1];
        dense_head<1>(h2, LD, H, p + L.pW3t, p + L.pb3, L.A, acc, lane);
        const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int r = 0; r < 4; r++) q[(g * 4 + r) * DQN_LDQ + r16] = acc[0][r];
    }
    __syncthreads();
}

template <int ACT, int NT>
__global__ __launch_bounds__(256) void dqn_act_kernel(const float *__restrict__ params, PLayout L, const float *__restrict__ obs, int64_t n, float eps,
                                                      uint32_t rng_seed, uint32_t rng_step, uint32_t env_offset, int32_t *__restrict__ actions_out,
                                                      float *__restrict__ q_out) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], h1[16 * LD], h2[16 * LD], q[16 * DQN_LDQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A;
    const int64_t n_tiles = (n + 15) >> 4;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(obs, row0, n, L.D, X, tid);
        __syncthreads();
        dqn_q_tile<ACT, NT>(params, L, X, h1, h2, q, lane, wave);
        if (tid < 16 && row0 + tid < n) {  // tma_egreedy_actions' rule on this row
            const int64_t r = row0 + tid;
            const uint32_t env = env_offset + (uint32_t)r;
            const float *qr = q + tid * DQN_LDQ;
            int a = 0;
            if (uniform01(mix32(rng_seed, env, rng_step)) < eps) {
                a = (int)(mix32(rng_seed ^ DQN_PICK_KEY, env, rng_step) % (uint32_t)A);
            } else {  // the first maximal column; a NaN never wins, a row of NaNs gives 0
                float m = qr[0];
                for (int c = 1; c < A; c++) {
                    const float v = qr[c];
                    if (v > m || (m != m && v == v)) m = v, a = c;
                }
            }
            actions_out[r] = a;
        }
        if (q_out) {
            for (int e = tid; e < 16 * A; e += 256) {
                const int row = e / A, c = e - row * A;
                if (row0 + row < n) q_out[(row0 + row) * A + c] = q[row * DQN_LDQ + c];
            }
        }
        __syncthreads();  // (the next tile overwrites X and q)
    }
}

struct DqnTdArgs {
    const float *params, *target;
    PLayout L;
    const float *obs, *next_obs, *dones, *rewards, *discounts;
    const int32_t *actions;
    int64_t n;
    float *slabs;   // [grid][L.vW1t]: the blocks' partial gradients of the pi segment
    double *parts;  // [grid][3]: loss sum, sum of Q taken, rows
    float *q_out;   // optional f32[n][A]: the online Q the loss used
};

template <int ACT, int NT>
__global__ __launch_bounds__(256) void dqn_td_kernel(DqnTdArgs a) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], Xn[16 * DQN_LDX], h1[16 * LD], h2[16 * LD], q[16 * DQN_LDQ], qn[16 * DQN_LDQ], dz3[16 * DQN_LDQ], rowstat[16 * 2];
    const PLayout &L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A, D = L.D, c0 = wave * 16 * NT;
    float *slab = a.slabs + (int64_t)blockIdx.x * L.vW1t;
    const float nf = (float)a.n;
    const int64_t n_tiles = (a.n + 15) >> 4;
    TileStats<2> stats;  // thread 0's: loss, Q taken
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(a.obs, row0, a.n, D, X, tid);
        dqn_load_tile(a.next_obs, row0, a.n, D, Xn, tid);
        __syncthreads();
        dqn_q_tile<ACT, NT>(a.target, L, Xn, h1, h2, qn, lane, wave);  // no gradient flows through it: h1, h2 are free again
        dqn_q_tile<ACT, NT>(a.params, L, X, h1, h2, q, lane, wave);
        if (tid < 16) {
            const int64_t r = row0 + tid;
            float ct = 0.0f, loss = 0.0f, qa = 0.0f;
            int act = -1;
            if (r < a.n) {
                float m = qn[tid * DQN_LDQ];
                for (int c = 1; c < A; c++) {
                    const float v = qn[tid * DQN_LDQ + c];
                    m = v > m ? v : m;
                }
                act = a.actions[r];  // only ever compared with column indices
                qa = __int_as_float(0x7FC00000);
                for (int c = 0; c < A; c++)
                    if (c == act) qa = q[tid * DQN_LDQ + c];
                const float y = a.rewards[r] + ((1.0f - a.dones[r]) * a.discounts[r]) * m;
                const float delta = qa - y, ad = fabsf(delta);
                loss = ad < 1.0f ? 0.5f * delta * delta : ad - 0.5f;   // smooth_l1, beta = 1
                ct = fminf(fmaxf(delta, -1.0f), 1.0f) / nf;            // (an action outside [0, A): NaN loss, and its cotangent lands in no column)
            }
            for (int c = 0; c < 16; c++) dz3[tid * DQN_LDQ + c] = (c < A && c == act) ? ct : 0.0f;
            rowstat[2 * tid] = loss, rowstat[2 * tid + 1] = qa;
        }
        if (a.q_out) {
            for (int e = tid; e < 16 * A; e += 256) {
                const int row = e / A, c = e - row * A;
                if (row0 + row < a.n) a.q_out[(row0 + row) * A + c] = q[row * DQN_LDQ + c];
            }
        }
        __syncthreads();
        if (tid == 0) stats.add_columns(row0, a.n, rowstat);
        dqn_wgrad(h2, LD, H, dz3, DQN_LDQ, A, slab + L.pW3t, first, lane, wave);
        dqn_bgrad(dz3, DQN_LDQ, A, slab + L.pb3, first, tid);
        __syncthreads();
        dqn_bwd_input<ACT, NT>(dz3, DQN_LDQ, A, a.params + L.pW3, H, h2, LD, lane, c0);  // h2 := dz2
        __syncthreads();
        dqn_wgrad(h1, LD, H, h2, LD, H, slab + L.pW2t, first, lane, wave);
        dqn_bgrad(h2, LD, H, slab + L.pb2, first, tid);
        __syncthreads();
        dqn_bwd_input<ACT, NT>(h2, LD, H, a.params + L.pW2, H, h1, LD, lane, c0);  // h1 := dz1
        __syncthreads();
        dqn_wgrad(X, DQN_LDX, D, h1, LD, H, slab + L.pW1t, first, lane, wave);
        dqn_bgrad(h1, LD, H, slab + L.pb1, first, tid);
        __syncthreads();  // (the next tile overwrites every buffer)
        first = false;
    }
    if (tid == 0) stats.store<3>(a.parts);
}

__global__ __launch_bounds__(256) void dqn_reduce_kernel(const float *__restrict__ slabs, const double *__restrict__ parts, int nb, int n_pi, int P,
                                                         float *__restrict__ grad, double *__restrict__ stats) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < P; e += gridDim.x * 256) {
        float s = 0.0f;
        if (e < n_pi) {
            s = slabs[e];
            for (int b = 1; b < nb; b++) s += slabs[(int64_t)b * n_pi + e];
        }
        grad[e] = s;
    }
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
        double s0 = parts[0], s1 = parts[1], s2 = parts[2];
        for (int b = 1; b < nb; b++) s0 += parts[3 * b], s1 += parts[3 * b + 1], s2 += parts[3 * b + 2];
        stats[0] = s0, stats[1] = s1, stats[2] = s2;
    }
}

static inline int dqn_td_grid(int64_t n) {
    const int64_t tiles = (n + 15) >> 4;
    return (int)(tiles < DQN_GRID_CAP ? tiles : DQN_GRID_CAP);
}
static inline int64_t dqn_parts_bytes(int grid) { return ((int64_t)grid * 3 * 8 + 15) & ~(int64_t)15; }

}  // namespace tma

using namespace tma;

// the shapes tma_dqn_* take: every refusal before any HIP call
static int dqn_check(const tma_policy_dims *d, const char *who) {
    if (!d) return fail(TMA_ERR_INVALID, "%s: null argument (dims)", who);
    const int rc = tma_check_policy_dims(d);
    if (rc) return rc;
    if (d->continuous) return fail(TMA_ERR_INVALID, "%s: a Box action space has no Q head (continuous must be 0)", who);
    if (d->mfma_dtype != 0) return fail(TMA_ERR_INVALID, "%s: mfma_dtype %d is not supported (the DQN kernels are exact f32: mfma_dtype 0)", who, d->mfma_dtype);
    if (d->hidden != 64 && d->hidden != 128 && d->hidden != 256) return fail(TMA_ERR_INVALID, "%s: hidden %d is not one of 64, 128, 256", who, d->hidden);
    if (d->act_dim < 2 || d->act_dim > 16) return fail(TMA_ERR_INVALID, "%s: act_dim %d is outside [2, 16]", who, d->act_dim);
    if (d->obs_dim < 1 || d->obs_dim > DQN_MAX_OBS) return fail(TMA_ERR_INVALID, "%s: obs_dim %d is outside [1, %d]", who, d->obs_dim, DQN_MAX_OBS);
    return TMA_OK;
}
static PLayout dqn_layout(const tma_policy_dims *d) { return make_layout(d->obs_dim, d->hidden, d->act_dim, 0, 0, d->activation); }

extern "C" {

int tma_dqn_act(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, double eps, uint32_t rng_seed, uint32_t rng_step,
                uint32_t env_offset, int32_t *actions_out, float *q_out, void *stream) {
    int rc = dqn_check(d, "tma_dqn_act");
    if (rc) return rc;
    if (!params || !obs || !actions_out) return fail(TMA_ERR_INVALID, "tma_dqn_act: null argument (params, obs or actions_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_dqn_act: n must be at least 1 (got %lld)", (long long)n);
    if (!(eps >= 0.0 && eps <= 1.0)) return fail(TMA_ERR_INVALID, "tma_dqn_act: eps %g is outside [0, 1]", eps);
    if ((rc = tile_set_device(d->device))) return rc;
    const PLayout L = dqn_layout(d);
    const int64_t tiles = (n + 15) >> 4;
    const dim3 grid((unsigned)(tiles < DQN_ACT_GRID_CAP ? tiles : DQN_ACT_GRID_CAP)), block(256);
    TILE_DISPATCH(dqn_act_kernel, L, (k<<<grid, block, 0, (hipStream_t)stream>>>(params, L, obs, n, (float)eps, rng_seed, rng_step, env_offset, actions_out, q_out)));
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int64_t tma_dqn_workspace_bytes(const tma_policy_dims *d, int64_t n) {
    if (dqn_check(d, "tma_dqn_workspace_bytes")) return 0;
    if (n < 1) {
        fail(TMA_ERR_INVALID, "tma_dqn_workspace_bytes: n must be at least 1 (got %lld)", (long long)n);
        return 0;
    }
    const PLayout L = dqn_layout(d);
    const int grid = dqn_td_grid(n);
    return dqn_parts_bytes(grid) + (int64_t)grid * L.vW1t * 4;
}

int tma_dqn_td_grad(const float *params, const float *target_params, const tma_policy_dims *d, const float *obs, const int32_t *actions,
                    const float *next_obs, const float *dones, const float *rewards, const float *discounts, int64_t n, float *grad_out,
                    double *stats_out, float *q_out, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = dqn_check(d, "tma_dqn_td_grad");
    if (rc) return rc;
    if (!params || !target_params || !obs || !actions || !next_obs || !dones || !rewards || !discounts || !grad_out)
        return fail(TMA_ERR_INVALID, "tma_dqn_td_grad: null argument (params, target_params, obs, actions, next_obs, dones, rewards, discounts or grad_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_dqn_td_grad: n must be at least 1 (got %lld)", (long long)n);
    const int64_t need = tma_dqn_workspace_bytes(d, n);
    if (!workspace || workspace_bytes < need)
        return fail(TMA_ERR_INVALID, "tma_dqn_td_grad: workspace of %lld bytes, tma_dqn_workspace_bytes reports %lld", (long long)(workspace ? workspace_bytes : 0),
                    (long long)need);
    if ((rc = tile_set_device(d->device))) return rc;
    const PLayout L = dqn_layout(d);
    const int grid = dqn_td_grid(n);
    double *parts = static_cast<double *>(workspace);
    float *slabs = reinterpret_cast<float *>(static_cast<char *>(workspace) + dqn_parts_bytes(grid));
    const DqnTdArgs a{params, target_params, L, obs, next_obs, dones, rewards, discounts, actions, n, slabs, parts, q_out};
    hipStream_t s = (hipStream_t)stream;
    TILE_DISPATCH(dqn_td_kernel, L, (k<<<dim3((unsigned)grid), dim3(256), 0, s>>>(a)));
    TMA_LAUNCH_CHECK();
    const int rb = (int)ceil_div(L.P, 256);
    dqn_reduce_kernel<<<dim3((unsigned)(rb < 256 ? rb : 256)), dim3(256), 0, s>>>(slabs, parts, grid, L.vW1t, L.P, grad_out, stats_out);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int tma_dqn_target_update(const float *params, float *target_params, const tma_policy_dims *d, double tau, void *stream) {
    int rc = dqn_check(d, "tma_dqn_target_update");
    if (rc) return rc;
    if (!params || !target_params) return fail(TMA_ERR_INVALID, "tma_dqn_target_update: null argument (params or target_params)");
    if (!(tau > 0.0 && tau <= 1.0)) return fail(TMA_ERR_INVALID, "tma_dqn_target_update: tau %g is outside (0, 1]", tau);
    if (params == target_params) return fail(TMA_ERR_INVALID, "tma_dqn_target_update: params and target_params are the same buffer");
    if ((rc = tile_set_device(d->device))) return rc;
    if ((rc = tma_polyak_update(params, target_params, dqn_layout(d).P, tau, stream))) return rc;
    return tma_policy_sync(target_params, d, stream);  // the derived copies the policy kernels read (the DQN kernels read none of the target's)
}

double tma_dqn_epsilon(const tma_dqn_hparams *hp, int64_t num_timesteps) {
    if (!hp) return 0.0;
    if (num_timesteps < hp->learning_starts) return 1.0;  // SB3's uniform warm-up
    const double total = hp->total_timesteps > 0 ? (double)hp->total_timesteps : 1.0;
    const double progress = 1.0 - (1.0 - (double)num_timesteps / total);  // SB3 get_linear_fn on progress_remaining = 1 - t / total
    if (progress > hp->exploration_fraction) return hp->exploration_final_eps;
    return hp->exploration_initial_eps + progress * (hp->exploration_final_eps - hp->exploration_initial_eps) / hp->exploration_fraction;
}

int tma_dqn_iterations_local(tma_env *env, float *params, float *target_params, const tma_policy_dims *d, const tma_replay *rb, const tma_dqn_buffers *b,
                             const tma_dqn_hparams *hp, tma_dqn_counters *c, int n_iters, void *stream) {
    int rc = dqn_check(d, "tma_dqn_iterations_local");
    if (rc) return rc;
    if (!env || !params || !target_params || !rb || !b || !hp || !c) return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: null argument");
    if (!b->last_obs || !b->actions || !b->step_obs || !b->rewards || !b->term || !b->trunc || !b->term_obs || !b->s_obs || !b->s_actions || !b->s_next_obs ||
        !b->s_dones || !b->s_rewards || !b->s_discounts || !b->grad || !b->exp_avg || !b->exp_avg_sq || !b->td_workspace || !b->opt_workspace)
        return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: a buffer of tma_dqn_buffers is null");
    if (n_iters < 1) return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: n_iters must be at least 1 (got %d)", n_iters);
    if (hp->train_freq < 1 || hp->batch_size < 1 || hp->target_update_interval < 1 || hp->gradient_steps == 0 || hp->gradient_steps < -1)
        return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: train_freq, batch_size and target_update_interval must be at least 1, gradient_steps >= 1 or -1");
    if (!(hp->exploration_fraction > 0.0 && hp->exploration_fraction <= 1.0))
        return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: exploration_fraction %g is outside (0, 1]", hp->exploration_fraction);
    if (rb->continuous || rb->obs_dim != d->obs_dim || rb->capacity < 1 || rb->n_envs < 1)
        return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: the replay view must be Discrete, of the policy's obs_dim, with capacity and n_envs >= 1");
    if (c->pos < 0 || c->pos >= rb->capacity || c->num_timesteps < 0 || c->n_calls < 0 || c->adam_step < 0)
        return fail(TMA_ERR_INVALID, "tma_dqn_iterations_local: counters out of range (pos %lld of %d rows)", (long long)c->pos, rb->capacity);
    const int64_t N = rb->n_envs;
    const int64_t every = hp->target_update_interval / N > 1 ? hp->target_update_interval / N : 1;
    const int grad_steps = hp->gradient_steps < 0 ? hp->train_freq : hp->gradient_steps;
    for (int it = 0; it < n_iters; it++) {
        for (int k = 0; k < hp->train_freq; k++) {
            const double eps = tma_dqn_epsilon(hp, c->num_timesteps);
            if ((rc = tma_dqn_act(params, d, b->last_obs, N, eps, hp->rng_seed, c->collect_step, hp->env_offset, b->actions, nullptr, stream))) return rc;
            if ((rc = offpolicy_collect_step(env, rb, b, c, TMA_ACT_I32, stream))) return rc;
            if (c->n_calls % every == 0 && (rc = tma_dqn_target_update(params, target_params, d, hp->tau, stream))) return rc;
        }
        if (c->num_timesteps > hp->learning_starts) {
            for (int gs = 0; gs < grad_steps; gs++) {
                if ((rc = offpolicy_sample(rb, b, hp, c, stream))) return rc;
                c->draw += 1;
                if ((rc = tma_dqn_td_grad(params, target_params, d, b->s_obs, b->s_actions, b->s_next_obs, b->s_dones, b->s_rewards, b->s_discounts, hp->batch_size,
                                          b->grad, b->stats, nullptr, b->td_workspace, b->td_workspace_bytes, stream)))
                    return rc;
                // last_count 0: the global step, which takes the norm of `grad` itself (no PPO gradient reduction left partials behind)
                if ((rc = tma_ppo_adam_step_local(params, b->grad, b->exp_avg, b->exp_avg_sq, d, c->adam_step + 1, hp->learning_rate, 0.9, 0.999, 1e-8,
                                                  hp->max_grad_norm, b->opt_workspace, stream, 0)))
                    return rc;
                c->adam_step += 1;
                c->n_updates += 1;
            }
        }
    }
    return TMA_OK;
}

}  // extern "C"
