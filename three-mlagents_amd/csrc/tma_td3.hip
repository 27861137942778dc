// tma_td3.hip -- SB3's TD3 on the device (ABI 227): tma_td3_param_offsets, tma_td3_act, tma_td3_critic_grad, tma_td3_actor_grad,
// tma_td3_workspace_bytes, tma_td3_iterations_local.  DESIGN.md section 19.
// Four flat [in][out] f32 buffers in SB3's tensor order: the actor (actor.mu.{0,2,4}: W1[D][H] b1 W2[H][H] b2 Wmu[H][A] bmu), the actor target,
// the critic pair and the critic target (tma_sac.hip's critic layout).  No derived copies.
//
// Unit of work, as in tma_sac.hip: ONE workgroup of four waves owns a tile of 16 rows, the tile's activations live in LDS, a barrier separates the
// layers.  td3_actor_tile is the ONE actor forward: tma_td3_act and both gradient kernels run it on the same thread layout, so a row's mu has the
// same bits in all three, whatever the batch it came in.
//
// tma_td3_critic_grad, launch 1 (td3_critic_kernel), per tile: target actor on next_obs -> a' = clamp(tanh(mu') + clamp(noise z, -c, c), -1, 1) ->
// both target critics on (next_obs | a') -> y;  then for each critic in turn: forward on (obs | a_replay), cotangent 2 (Q - y) / n, dW3 / db3, dz2
// (in place of h2), dW2 / db2, dz1 (in place of h1), dW1 / db1 into the block's slab.  tma_td3_actor_grad, launch 1 (td3_actor_kernel), per tile:
// actor forward on obs -> a = tanh(mu) -> qf0 on (obs | a), its hidden activations kept -> -1 / n down qf0's input gradient to the action rows of
// its W1 -> through the tanh -> the actor's backward into the slab.  Launch 2 of either (sac_reduce_kernel) folds the slabs and the float64
// partials in block order.  No float atomics; a gradient element is summed over the rows of a tile in row order, a block's tiles in order, the
// blocks in order: equal inputs give equal bits.
// Shared: sac_q_tile, critic_row_stats and a gradient entry's frame sac_grad_run (tma_sac_tile.h); mlp_trunk_tile, TileStats, TILE_DISPATCH and
// the loop's collect step and sample (tma_dqn_tile.h).  NOT shared, on a measurement: the two gradient kernels spell out the backward chains that
// tma_sac_tile.h holds as q_backward_tile, q_action_grad_tile and trunk_backward_tile.  Through those functions the same operations compiled to
// a different register allocation, and at H = 256 the kernels ran 0.3 - 0.6 % slower than written out (SAC's did not); the text here and there
// must be kept in step by hand.
#include "tma_sac_tile.h"

namespace tma {

constexpr uint32_t TD3_KEY_COLLECT = 0x7D3C011Eu, TD3_KEY_TARGET = 0x7D37A26Eu;

// the actor buffer is the front of SAC's (there is no log_std head): n_actor ends behind bmu
__host__ __device__ inline SacLayout td3_layout(int D, int A, int H, int act) {
    SacLayout L = sac_layout(D, A, H, act);
    L.n_actor = L.aWls;
    L.aWls = L.abls = -1;
    return L;
}

// THE actor forward: head[16][DQN_LDQ], columns j < A = mu_j before the tanh (the other columns are zeros); h1, h2 keep the hidden activations.
// Every thread of the workgroup calls it (it holds barriers); X[.][0 .. D) must be complete; on return head, h1, h2 are visible to every thread.
template <int ACT, int NT>
__device__ __forceinline__ void td3_actor_tile(const float *__restrict__ p, const SacLayout &L, const float *X, float *h1, float *h2, float *head, int lane,
                                               int wave) {
    constexpr int H = 64 * NT, LD = H + 2;
    mlp_trunk_tile<ACT, NT>(X, L.D, p, L.aW1, L.ab1, L.aW2, L.ab2, h1, h2, lane, wave);
    if (wave == 0) {
        const int r16 = lane & 15, g = lane >> 4, A = L.A;
        const bool ok = r16 < A;
        const float *W = p + L.aWmu;
        const float bias = ok ? p[L.abmu + r16] : 0.0f;
        f32x4 acc = f32x4{bias, bias, bias, bias};
        for (int ks = 0; ks < (H >> 2); ks++) {
            const int k = 4 * ks + g;
            const float w = ok ? W[k * A + r16] : 0.0f;
            acc = mfma16(h2[r16 * LD + k], w, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) head[(g * 4 + r) * DQN_LDQ + r16] = acc[r];
    }
    __syncthreads();
}

__device__ __forceinline__ void td3_store_head(float *__restrict__ head_out, const float *head, int64_t row0, int64_t n, int A, int tid) {
    for (int e = tid; e < 16 * A; e += 256) {
        const int row = e / A, c = e - row * A;
        if (row0 + row < n) head_out[(row0 + row) * A + c] = head[row * DQN_LDQ + c];
    }
}

__device__ __forceinline__ float td3_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

struct Td3Noise {
    float mean[SAC_MAX_A], sigma[SAC_MAX_A];
};

// a = tanh(mu), or in the noisy mode clamp(tanh(mu) + mean_j + sigma_j z, -1, 1) (SB3: the action noise is added to the squashed action and clipped)
template <int ACT, int NT>
__global__ __launch_bounds__(256) void td3_act_kernel(const float *__restrict__ actor, SacLayout L, const float *__restrict__ obs, int64_t n, int noisy,
                                                      Td3Noise an, uint32_t seed, uint32_t draw, uint32_t row_offset, const float *__restrict__ noise_in,
                                                      float *__restrict__ actions_out, float *__restrict__ noise_out, float *__restrict__ head_out) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], h1[16 * LD], h2[16 * LD], head[16 * DQN_LDQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A;
    const int64_t n_tiles = (n + 15) >> 4;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(obs, row0, n, L.D, X, tid);
        __syncthreads();
        td3_actor_tile<ACT, NT>(actor, L, X, h1, h2, head, lane, wave);
        if (tid < 16 && row0 + tid < n) {
            const int64_t r = row0 + tid;
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++) {
                if (j < A) {
                    float a = tanhf(head[tid * DQN_LDQ + j]), z = 0.0f;
                    if (noisy) {
                        z = noise_in ? noise_in[r * A + j] : sac_normal(seed ^ TD3_KEY_COLLECT, row_offset + (uint32_t)r, draw, j);
                        a = td3_clamp(a + (an.mean[j] + an.sigma[j] * z), -1.0f, 1.0f);
                    }
                    actions_out[r * A + j] = a;
                    if (noise_out) noise_out[r * A + j] = z;
                }
            }
        }
        if (head_out) td3_store_head(head_out, head, row0, n, A, tid);
        __syncthreads();  // (the next tile overwrites X and head)
    }
}

struct Td3CriticArgs {
    const float *actor_target, *critic, *target;
    SacLayout L;
    const float *obs, *actions, *next_obs, *dones, *rewards, *discounts, *noise_in;
    int64_t n;
    uint32_t seed, draw;
    float policy_noise, noise_clip;
    float *slabs;    // [grid][2 n_q]
    double *parts;   // [grid][4]: sum of (Q0 - y)^2 + (Q1 - y)^2, sum Q0, sum Q1, rows
    float *q_out, *target_out, *noise_out, *head_out;
};

template <int ACT, int NT>
__global__ __launch_bounds__(256) void td3_critic_kernel(Td3CriticArgs a) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], Xn[16 * DQN_LDX], h1[16 * LD], h2[16 * LD], head[16 * DQN_LDQ], qt[32], qv[16], yv[16], dz3[16 * DQN_LDQ], rowstat[16 * 4];
    const SacLayout &L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A, D = L.D, c0 = wave * 16 * NT;
    float *slab = a.slabs + (int64_t)blockIdx.x * 2 * L.n_q;
    const float nf = (float)a.n;
    const int64_t n_tiles = (a.n + 15) >> 4;
    TileStats<3> stats;  // thread 0's: critic loss, Q0, Q1
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(a.obs, row0, a.n, D, X, tid);
        dqn_load_tile(a.actions, row0, a.n, A, X + D, tid);  // (obs | a_replay): SB3's concatenation
        dqn_load_tile(a.next_obs, row0, a.n, D, Xn, tid);
        __syncthreads();
        td3_actor_tile<ACT, NT>(a.actor_target, L, Xn, h1, h2, head, lane, wave);
        if (tid < 16) {  // target-policy smoothing: a' = clamp(tanh(mu') + clamp(policy_noise z, -clip, clip), -1, 1)
            const int64_t r = row0 + tid;
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++) {
                if (j < A) {
                    float an = 0.0f;
                    if (r < a.n) {
                        const float z = a.noise_in ? a.noise_in[r * A + j] : sac_normal(a.seed ^ TD3_KEY_TARGET, (uint32_t)r, a.draw, j);
                        if (a.noise_out) a.noise_out[r * A + j] = z;
                        const float eps = td3_clamp(a.policy_noise * z, -a.noise_clip, a.noise_clip);
                        an = td3_clamp(tanhf(head[tid * DQN_LDQ + j]) + eps, -1.0f, 1.0f);
                    }
                    Xn[tid * DQN_LDX + D + j] = an;
                }
            }
        }
        if (a.head_out) td3_store_head(a.head_out, head, row0, a.n, A, tid);
        __syncthreads();
        sac_q_tile<ACT, NT>(a.target, L, Xn, h1, h2, qt, lane, wave);
        sac_q_tile<ACT, NT>(a.target + L.n_q, L, Xn, h1, h2, qt + 16, lane, wave);
        if (tid < 16) {
            const int64_t r = row0 + tid;
            float y = 0.0f;
            if (r < a.n) {
                y = a.rewards[r] + ((1.0f - a.dones[r]) * a.discounts[r]) * fminf(qt[tid], qt[16 + tid]);
                if (a.target_out) a.target_out[r] = y;
            }
            yv[tid] = y;
        }
        __syncthreads();
        for (int i = 0; i < 2; i++) {
            const float *cp = a.critic + (int64_t)i * L.n_q;
            float *sl = slab + (int64_t)i * L.n_q;
            sac_q_tile<ACT, NT>(cp, L, X, h1, h2, qv, lane, wave);
            if (tid < 16) {
                const int64_t r = row0 + tid;
                float ct = 0.0f, loss = 0.0f, q = 0.0f;
                if (r < a.n) {
                    q = qv[tid];
                    const float delta = q - yv[tid];
                    loss = delta * delta;         // SB3's TD3: sum(F.mse_loss(...)), no 1/2
                    ct = (2.0f * delta) / nf;
                    if (a.q_out) a.q_out[r * 2 + i] = q;
                }
                for (int c = 0; c < 16; c++) dz3[tid * DQN_LDQ + c] = c == 0 ? ct : 0.0f;
                rowstat[4 * tid + 2 * i] = loss, rowstat[4 * tid + 2 * i + 1] = q;
            }
            __syncthreads();
            // (tma_sac_tile.h's q_backward_tile written out: through the function these kernels measured 0.3 - 0.6 % slower at H = 256)
            dqn_wgrad(h2, LD, H, dz3, DQN_LDQ, 1, sl + L.qW3, first, lane, wave);
            dqn_bgrad(dz3, DQN_LDQ, 1, sl + L.qb3, first, tid);
            __syncthreads();
            for (int e = tid; e < 16 * H; e += 256) {  // h2 := dz2 = dz3 W3^T act'(h2): one output column, so one product per element
                const int row = e / H, k = e - row * H;
                h2[row * LD + k] = act_bwd<ACT>(dz3[row * DQN_LDQ] * cp[L.qW3 + k], h2[row * LD + k]);
            }
            __syncthreads();
            dqn_wgrad(h1, LD, H, h2, LD, H, sl + L.qW2, first, lane, wave);
            dqn_bgrad(h2, LD, H, sl + L.qb2, first, tid);
            __syncthreads();
            sac_bwd_input_t<ACT, NT>(h2, LD, H, cp + L.qW2, h1, LD, lane, c0);  // h1 := dz1
            __syncthreads();
            dqn_wgrad(X, DQN_LDX, D + A, h1, LD, H, sl + L.qW1, first, lane, wave);
            dqn_bgrad(h1, LD, H, sl + L.qb1, first, tid);
            __syncthreads();  // (the next critic / tile overwrites every buffer)
        }
        if (tid == 0) stats.add(row0, a.n, critic_row_stats(rowstat));
        __syncthreads();  // (rowstat is rewritten by the next tile)
        first = false;
    }
    if (tid == 0) stats.store<4>(a.parts);
}

struct Td3ActorArgs {
    const float *actor, *critic;
    SacLayout L;
    const float *obs;
    int64_t n;
    float *slabs;    // [grid][n_actor]
    double *parts;   // [grid][4]: sum of -Q0, rows, (unused), (unused)
    float *actions_out, *head_out;
};

template <int ACT, int NT>
__global__ __launch_bounds__(256) void td3_actor_kernel(Td3ActorArgs a) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], ha1[16 * LD], ha2[16 * LD], hq1[16 * LD], hq2[16 * LD], head[16 * DQN_LDQ], dzh[16 * DQN_LDQ], qv[16], dzq[16],
        ats[16 * SAC_MAX_A], dA[16 * SAC_MAX_A];
    const SacLayout &L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A, D = L.D, c0 = wave * 16 * NT;
    float *slab = a.slabs + (int64_t)blockIdx.x * L.n_actor;
    const float nf = (float)a.n;
    const int64_t n_tiles = (a.n + 15) >> 4;
    TileStats<1> stats;  // thread 0's: the sum of -Q0
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(a.obs, row0, a.n, D, X, tid);
        __syncthreads();
        td3_actor_tile<ACT, NT>(a.actor, L, X, ha1, ha2, head, lane, wave);
        if (tid < 16) {
            const int64_t r = row0 + tid;
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++) {
                float ap = 0.0f;
                if (j < A && r < a.n) {
                    ap = tanhf(head[tid * DQN_LDQ + j]);
                    if (a.actions_out) a.actions_out[r * A + j] = ap;
                }
                if (j < A) X[tid * DQN_LDX + D + j] = ap;
                ats[tid * SAC_MAX_A + j] = ap;
            }
        }
        if (a.head_out) td3_store_head(a.head_out, head, row0, a.n, A, tid);
        __syncthreads();
        sac_q_tile<ACT, NT>(a.critic, L, X, hq1, hq2, qv, lane, wave);  // qf0 alone (SB3: critic.q1_forward)
        if (tid < 16) dzq[tid] = row0 + tid < a.n ? -1.0f / nf : 0.0f;
        if (tid == 0) stats.add(row0, a.n, [&](int row, double(&v)[1]) { v[0] = -(double)qv[row]; });
        __syncthreads();
        // (tma_sac_tile.h's q_action_grad_tile<.., 1> and, below, trunk_backward_tile written out: see td3_critic_kernel)
        for (int e = tid; e < 16 * H; e += 256) {  // hq2 := dz2 of qf0 (its head has one column: one product per element)
            const int row = e / H, k = e - row * H;
            hq2[row * LD + k] = act_bwd<ACT>(dzq[row] * a.critic[L.qW3 + k], hq2[row * LD + k]);
        }
        __syncthreads();
        sac_bwd_input_t<ACT, NT>(hq2, LD, H, a.critic + L.qW2, hq1, LD, lane, c0);  // hq1 := dz1
        __syncthreads();
        {  // dQ0/da through the action rows of qf0's W1 (no critic weight gradient is formed): thread (row, j), h in order
            const int row = tid >> 4, j = tid & 15;
            if (j < A) {
                const float *w = a.critic + L.qW1 + (int64_t)(D + j) * H;
                float s = 0.0f;
                for (int h = 0; h < H; h++) s += hq1[row * LD + h] * w[h];
                dA[row * SAC_MAX_A + j] = s;
            }
        }
        __syncthreads();
        if (tid < 16) {  // through the tanh into the head cotangent
            const bool in = row0 + tid < a.n;
            for (int c = 0; c < 16; c++) dzh[tid * DQN_LDQ + c] = 0.0f;
            for (int j = 0; j < A && in; j++) {
                const float av = ats[tid * SAC_MAX_A + j];
                dzh[tid * DQN_LDQ + j] = dA[tid * SAC_MAX_A + j] * (1.0f - av * av);
            }
        }
        __syncthreads();
        dqn_wgrad(ha2, LD, H, dzh, DQN_LDQ, A, slab + L.aWmu, first, lane, wave);
        dqn_bgrad(dzh, DQN_LDQ, A, slab + L.abmu, first, tid);
        __syncthreads();
        for (int e = tid; e < 16 * H; e += 256) {  // ha2 := dz2 = dmu Wmu^T act'(ha2), columns in order
            const int row = e / H, k = e - row * H;
            float s = 0.0f;
            for (int j = 0; j < A; j++) s += dzh[row * DQN_LDQ + j] * a.actor[L.aWmu + k * A + j];
            ha2[row * LD + k] = act_bwd<ACT>(s, ha2[row * LD + k]);
        }
        __syncthreads();
        dqn_wgrad(ha1, LD, H, ha2, LD, H, slab + L.aW2, first, lane, wave);
        dqn_bgrad(ha2, LD, H, slab + L.ab2, first, tid);
        __syncthreads();
        sac_bwd_input_t<ACT, NT>(ha2, LD, H, a.actor + L.aW2, ha1, LD, lane, c0);  // ha1 := dz1
        __syncthreads();
        dqn_wgrad(X, DQN_LDX, D, ha1, LD, H, slab + L.aW1, first, lane, wave);
        dqn_bgrad(ha1, LD, H, slab + L.ab1, first, tid);
        __syncthreads();  // (the next tile overwrites every buffer)
        first = false;
    }
    if (tid == 0) stats.store<4>(a.parts);
}

static SacLayout td3_layout_of(const tma_sac_dims *d) { return td3_layout(d->obs_dim, d->act_dim, d->hidden, d->activation); }

}  // namespace tma

using namespace tma;

extern "C" {

int tma_td3_param_offsets(const tma_sac_dims *d, tma_td3_offsets *out) {
    const int rc = sac_check(d, "tma_td3_param_offsets");
    if (rc) return rc;
    if (!out) return fail(TMA_ERR_INVALID, "tma_td3_param_offsets: null argument (out)");
    const SacLayout L = td3_layout_of(d);
    out->a_W1 = L.aW1, out->a_b1 = L.ab1, out->a_W2 = L.aW2, out->a_b2 = L.ab2, out->a_Wmu = L.aWmu, out->a_bmu = L.abmu, out->n_actor = L.n_actor;
    out->q_W1 = L.qW1, out->q_b1 = L.qb1, out->q_W2 = L.qW2, out->q_b2 = L.qb2, out->q_W3 = L.qW3, out->q_b3 = L.qb3;
    out->n_q = L.n_q, out->n_critic = 2 * L.n_q;
    return TMA_OK;
}

int tma_td3_act(const float *actor, const tma_sac_dims *d, const float *obs, int64_t n, int mode, const tma_td3_noise *action_noise, uint32_t seed,
                uint32_t draw, uint32_t row_offset, const float *noise_in, float *actions_out, float *noise_out, float *head_out, void *stream) {
    int rc = sac_check(d, "tma_td3_act");
    if (rc) return rc;
    if (mode != TMA_TD3_DETERMINISTIC && mode != TMA_TD3_NOISY && mode != TMA_TD3_UNIFORM)
        return fail(TMA_ERR_INVALID, "tma_td3_act: mode %d is none of TMA_TD3_DETERMINISTIC (0), TMA_TD3_NOISY (1), TMA_TD3_UNIFORM (2)", mode);
    if (!actions_out) return fail(TMA_ERR_INVALID, "tma_td3_act: null argument (actions_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_td3_act: n must be at least 1 (got %lld)", (long long)n);
    if (mode == TMA_TD3_UNIFORM) {
        if (noise_in || noise_out || head_out)
            return fail(TMA_ERR_INVALID, "tma_td3_act: the uniform mode reads no net and no noise: noise_in, noise_out and head_out must be NULL");
        // SAC's warm-up arithmetic, through its own entry: equal (seed, draw, row_offset) give the bits tma_sac_act gives
        return tma_sac_act(nullptr, d, nullptr, n, TMA_SAC_UNIFORM, seed, draw, row_offset, nullptr, actions_out, nullptr, nullptr, nullptr, stream);
    }
    if (!actor || !obs) return fail(TMA_ERR_INVALID, "tma_td3_act: null argument (actor or obs)");
    Td3Noise an{};
    if (mode == TMA_TD3_DETERMINISTIC) {
        if (noise_in) return fail(TMA_ERR_INVALID, "tma_td3_act: the deterministic mode takes no noise_in");
    } else {
        if (!action_noise) return fail(TMA_ERR_INVALID, "tma_td3_act: the noisy mode needs action_noise (mean and sigma)");
        for (int j = 0; j < d->act_dim; j++) {
            const float m = action_noise->mean[j], s = action_noise->sigma[j];
            if (!(m == m) || !(s >= 0.0f)) return fail(TMA_ERR_INVALID, "tma_td3_act: action_noise column %d: mean %g is NaN or sigma %g is negative or NaN", j, m, s);
            an.mean[j] = m, an.sigma[j] = s;
        }
    }
    if ((rc = tile_set_device(d->device))) return rc;
    const SacLayout L = td3_layout_of(d);
    const int64_t tiles = (n + 15) >> 4;
    const dim3 grid((unsigned)(tiles < SAC_ACT_GRID_CAP ? tiles : SAC_ACT_GRID_CAP)), block(256);
    TILE_DISPATCH(td3_act_kernel, L, (k<<<grid, block, 0, (hipStream_t)stream>>>(actor, L, obs, n, mode == TMA_TD3_NOISY ? 1 : 0, an, seed, draw, row_offset, noise_in,
                                                                                 actions_out, noise_out, head_out)));
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int64_t tma_td3_workspace_bytes(const tma_sac_dims *d, int64_t n) {
    if (sac_check(d, "tma_td3_workspace_bytes")) return 0;
    if (n < 1) {
        fail(TMA_ERR_INVALID, "tma_td3_workspace_bytes: n must be at least 1 (got %lld)", (long long)n);
        return 0;
    }
    return sac_workspace_bytes_of(td3_layout_of(d), n);
}

int tma_td3_critic_grad(const float *actor_target, const float *critic, const float *critic_target, const tma_sac_dims *d, const float *obs, const float *actions,
                        const float *next_obs, const float *dones, const float *rewards, const float *discounts, int64_t n, double target_policy_noise,
                        double target_noise_clip, uint32_t seed, uint32_t draw, const float *noise_in, float *grad_out, double *stats_out, float *q_out,
                        float *target_out, float *noise_out, float *head_out, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = sac_check(d, "tma_td3_critic_grad");
    if (rc) return rc;
    if (!actor_target || !critic || !critic_target || !obs || !actions || !next_obs || !dones || !rewards || !discounts || !grad_out)
        return fail(TMA_ERR_INVALID,
                    "tma_td3_critic_grad: null argument (actor_target, critic, critic_target, obs, actions, next_obs, dones, rewards, discounts or grad_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_td3_critic_grad: n must be at least 1 (got %lld)", (long long)n);
    if (!(target_policy_noise >= 0.0) || !(target_noise_clip >= 0.0))
        return fail(TMA_ERR_INVALID, "tma_td3_critic_grad: target_policy_noise %g and target_noise_clip %g must be at least 0", target_policy_noise,
                    target_noise_clip);
    const SacLayout L = td3_layout_of(d);
    hipStream_t s = (hipStream_t)stream;
    return sac_grad_run("tma_td3_critic_grad", "tma_td3_workspace_bytes", d, L, n, workspace, workspace_bytes, 2 * L.n_q, 4, grad_out, stats_out, s,
                        [&](int grid, float *slabs, double *parts) {
                            const Td3CriticArgs a{actor_target, critic, critic_target, L, obs, actions, next_obs, dones, rewards, discounts, noise_in, n, seed, draw,
                                                  (float)target_policy_noise, (float)target_noise_clip, slabs, parts, q_out, target_out, noise_out, head_out};
                            TILE_DISPATCH(td3_critic_kernel, L, (k<<<dim3((unsigned)grid), dim3(256), 0, s>>>(a)));
                        });
}

int tma_td3_actor_grad(const float *actor, const float *critic, const tma_sac_dims *d, const float *obs, int64_t n, float *grad_out, double *stats_out,
                       float *actions_out, float *head_out, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = sac_check(d, "tma_td3_actor_grad");
    if (rc) return rc;
    if (!actor || !critic || !obs || !grad_out) return fail(TMA_ERR_INVALID, "tma_td3_actor_grad: null argument (actor, critic, obs or grad_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_td3_actor_grad: n must be at least 1 (got %lld)", (long long)n);
    const SacLayout L = td3_layout_of(d);
    hipStream_t s = (hipStream_t)stream;
    return sac_grad_run("tma_td3_actor_grad", "tma_td3_workspace_bytes", d, L, n, workspace, workspace_bytes, L.n_actor, 2, grad_out, stats_out, s,
                        [&](int grid, float *slabs, double *parts) {
                            const Td3ActorArgs a{actor, critic, L, obs, n, slabs, parts, actions_out, head_out};
                            TILE_DISPATCH(td3_actor_kernel, L, (k<<<dim3((unsigned)grid), dim3(256), 0, s>>>(a)));
                        });
}

int tma_td3_iterations_local(tma_env *env, float *actor, float *actor_target, float *critic, float *critic_target, const tma_sac_dims *d, const tma_replay *rb,
                             const tma_td3_buffers *b, const tma_td3_hparams *hp, tma_td3_counters *c, int n_iters, void *stream) {
    int rc = sac_check(d, "tma_td3_iterations_local");
    if (rc) return rc;
    if (!env || !actor || !actor_target || !critic || !critic_target || !rb || !b || !hp || !c)
        return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: null argument");
    if (!b->last_obs || !b->actions || !b->step_obs || !b->rewards || !b->term || !b->trunc || !b->term_obs || !b->s_obs || !b->s_actions || !b->s_next_obs ||
        !b->s_dones || !b->s_rewards || !b->s_discounts || !b->actor_grad || !b->actor_exp_avg || !b->actor_exp_avg_sq || !b->critic_grad || !b->critic_exp_avg ||
        !b->critic_exp_avg_sq || !b->critic_stats || !b->actor_stats || !b->workspace)
        return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: a buffer of tma_td3_buffers is null");
    if (n_iters < 1) return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: n_iters must be at least 1 (got %d)", n_iters);
    if (hp->train_freq < 1 || hp->batch_size < 1 || hp->policy_delay < 1 || hp->gradient_steps == 0 || hp->gradient_steps < -1)
        return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: train_freq, batch_size and policy_delay must be at least 1, gradient_steps >= 1 or -1");
    if (!(hp->target_policy_noise >= 0.0) || !(hp->target_noise_clip >= 0.0))
        return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: target_policy_noise %g and target_noise_clip %g must be at least 0", hp->target_policy_noise,
                    hp->target_noise_clip);
    if (!rb->continuous || rb->obs_dim != d->obs_dim || rb->act_dim != d->act_dim || rb->capacity < 1 || rb->n_envs < 1)
        return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: the replay view must be Box, of the dims' obs_dim and act_dim, with capacity and n_envs >= 1");
    if (c->pos < 0 || c->pos >= rb->capacity || c->num_timesteps < 0 || c->n_calls < 0 || c->critic_adam_step < 0 || c->actor_adam_step < 0 || c->n_updates < 0)
        return fail(TMA_ERR_INVALID, "tma_td3_iterations_local: counters out of range (pos %lld of %d rows)", (long long)c->pos, rb->capacity);
    const int64_t N = rb->n_envs;
    const int grad_steps = hp->gradient_steps < 0 ? hp->train_freq : hp->gradient_steps;
    const SacLayout L = td3_layout_of(d);
    const int64_t B = hp->batch_size;
    for (int it = 0; it < n_iters; it++) {
        for (int k = 0; k < hp->train_freq; k++) {
            const bool warm = c->num_timesteps < hp->learning_starts;  // SB3's uniform warm-up
            const int mode = warm ? TMA_TD3_UNIFORM : hp->use_action_noise ? TMA_TD3_NOISY : TMA_TD3_DETERMINISTIC;
            if ((rc = tma_td3_act(warm ? nullptr : actor, d, warm ? nullptr : b->last_obs, N, mode, &hp->action_noise, hp->rng_seed, c->collect_step, hp->env_offset,
                                  nullptr, b->actions, nullptr, nullptr, stream)))
                return rc;
            if ((rc = offpolicy_collect_step(env, rb, b, c, TMA_ACT_F32, stream))) return rc;
        }
        if (c->num_timesteps > hp->learning_starts) {
            for (int gs = 0; gs < grad_steps; gs++) {
                c->n_updates += 1;  // SB3 counts before it decides: the actor steps where n_updates % policy_delay == 0
                if ((rc = offpolicy_sample(rb, b, hp, c, stream))) return rc;
                if ((rc = tma_td3_critic_grad(actor_target, critic, critic_target, d, b->s_obs, b->s_actions, b->s_next_obs, b->s_dones, b->s_rewards, b->s_discounts, B,
                                              hp->target_policy_noise, hp->target_noise_clip, hp->rng_seed, c->draw, nullptr, b->critic_grad, b->critic_stats, nullptr,
                                              nullptr, nullptr, nullptr, b->workspace, b->workspace_bytes, stream)))
                    return rc;
                if ((rc = tma_adam_step_flat(critic, b->critic_grad, b->critic_exp_avg, b->critic_exp_avg_sq, 2 * (int64_t)L.n_q, c->critic_adam_step + 1,
                                             hp->learning_rate, 0.9, 0.999, 1e-8, stream)))
                    return rc;
                c->critic_adam_step += 1;
                c->draw += 1;
                if (c->n_updates % hp->policy_delay == 0) {
                    if ((rc = tma_td3_actor_grad(actor, critic, d, b->s_obs, B, b->actor_grad, b->actor_stats, nullptr, nullptr, b->workspace, b->workspace_bytes,
                                                 stream)))
                        return rc;
                    if ((rc = tma_adam_step_flat(actor, b->actor_grad, b->actor_exp_avg, b->actor_exp_avg_sq, L.n_actor, c->actor_adam_step + 1, hp->learning_rate, 0.9,
                                                 0.999, 1e-8, stream)))
                        return rc;
                    c->actor_adam_step += 1;
                    if ((rc = tma_polyak_update(critic, critic_target, 2 * (int64_t)L.n_q, hp->tau, stream))) return rc;
                    if ((rc = tma_polyak_update(actor, actor_target, L.n_actor, hp->tau, stream))) return rc;
                }
            }
        }
    }
    return TMA_OK;
}

}  // extern "C"
