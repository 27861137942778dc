// tma_sac.hip -- SB3's SAC on the device (ABI 226): tma_sac_act, tma_sac_critic_grad, tma_sac_actor_grad, tma_sac_ent_coef_grad,
// tma_adam_step_flat, tma_polyak_update, tma_sac_iterations_local.  DESIGN.md section 18.
// Three flat [in][out] f32 buffers in SB3's tensor order (tma_sac_param_offsets): the actor (latent_pi, mu, log_std), the two critics
// (qf0 then qf1, each over the concatenation obs | action), the critic target; log_ent_coef is one device float.  No derived copies: the input
// gradient of a hidden layer reads the [in][out] matrix itself, four consecutive dwords of a row per lane (sac_bwd_input_t).
//
// Unit of work, as in tma_dqn.hip: ONE workgroup of four waves owns a tile of 16 rows, a hidden layer's H columns are split over the waves, the
// tile's activations live in LDS, a barrier separates the layers.  sac_actor_tile is the ONE actor forward and sac_squash_row the ONE squash:
// tma_sac_act and both gradient kernels run them on the same thread layout, so a row's mu / log_std / action have the same bits in all three.
//
// tma_sac_critic_grad, launch 1 (sac_critic_kernel), per tile: actor forward on next_obs -> a', logp' -> both target critics on (next_obs | a')
// -> y;  then for each critic in turn: forward on (obs | a_replay), cotangent (Q - y) / n, dW3 / db3, dz2 (in place of h2), dW2 / db2, dz1 (in
// place of h1), dW1 / db1 into the block's slab.  tma_sac_actor_grad, launch 1 (sac_actor_kernel), per tile: actor forward on obs -> a_pi, logp_pi
// -> both critics on (obs | a_pi), whose hidden activations are all kept -> the winner of the min takes -1 / n -> both critics' input gradients
// down to the action rows of W1 -> through the squash and logp into the head cotangent -> the actor's backward into the slab.  Launch 2 of
// either (sac_reduce_kernel) folds the slabs and the float64 partials in block order.  No float atomics; a gradient element is summed over the
// rows of a tile in row order, a block's tiles in order, the blocks in order: equal inputs give equal bits.
// The layout, sac_bwd_input_t, sac_q_tile, q_backward_tile (one critic's backward), q_action_grad_tile (the critics' input gradients down to dQ/da),
// trunk_backward_tile (the actor's two hidden layers), sac_normal, the slab fold, the shape check and sac_grad_run (the frame of a gradient entry)
// live in tma_sac_tile.h, which tma_td3.hip shares (all but the three backward functions: see its head); mlp_trunk_tile, TileStats, TILE_DISPATCH and the native loop's collect step and sample in
// tma_dqn_tile.h, which tma_dqn.hip shares as well.
#include "tma_sac_tile.h"

namespace tma {

constexpr uint32_t SAC_KEY_COLLECT = 0xC011EC70u, SAC_KEY_NEXT = 0x4E787AC7u, SAC_KEY_PI = 0x5AC0A17Eu, SAC_KEY_UNIFORM = 0x0D1F0A3Bu;
constexpr float SAC_LS_MIN = -20.0f, SAC_LS_MAX = 2.0f, SAC_EPS = 1e-6f;

// THE actor forward: head[16][DQN_LDQ], columns j < A = mu_j, columns 8 + j = log_std_j before the clamp; h1, h2 keep the hidden activations.
// Every thread of the workgroup calls it (it holds barriers); X[.][0 .. D) must be complete; on return head, h1, h2 are visible to every thread.
template <int ACT, int NT>
__device__ __forceinline__ void sac_actor_tile(const float *__restrict__ p, const SacLayout &L, const float *X, float *h1, float *h2, float *head, int lane,
                                               int wave) {
    constexpr int H = 64 * NT, LD = H + 2;
    mlp_trunk_tile<ACT, NT>(X, L.D, p, L.aW1, L.ab1, L.aW2, L.ab2, h1, h2, lane, wave);
    if (wave == 0) {
        const int r16 = lane & 15, g = lane >> 4, j = r16 & 7, A = L.A;
        const bool ok = j < A;
        const float *W = p + (r16 < 8 ? L.aWmu : L.aWls), *b = p + (r16 < 8 ? L.abmu : L.abls);
        const float bias = ok ? b[j] : 0.0f;
        f32x4 acc = f32x4{bias, bias, bias, bias};
        for (int ks = 0; ks < (H >> 2); ks++) {
            const int k = 4 * ks + g;
            const float w = ok ? W[k * A + j] : 0.0f;
            acc = mfma16(h2[r16 * LD + k], w, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) head[(g * 4 + r) * DQN_LDQ + r16] = acc[r];
    }
    __syncthreads();
}

// THE squash of one row (SB3's SquashedDiagGaussianDistribution): from head_row (mu at [j], log_std at [8 + j]) and z[j]
//   ls = clamp(log_std, -20, 2), sd = exp(ls), u = mu + sd z, a = tanh(u), logp = sum_j (-z^2 / 2 - ls - log sqrt(2 pi)) - sum_j log(1 - a^2 + 1e-6)
// `deterministic`: z is taken as 0 (a = tanh(mu)).  Returns logp; a[j], sd[j] for j < A.
__device__ __forceinline__ float sac_squash_row(const float *head_row, int A, const float (&z)[SAC_MAX_A], float (&a)[SAC_MAX_A], float (&sd)[SAC_MAX_A]) {
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < SAC_MAX_A; j++) {
        a[j] = 0.0f, sd[j] = 0.0f;
        if (j < A) {
            const float ls = fminf(fmaxf(head_row[8 + j], SAC_LS_MIN), SAC_LS_MAX);
            sd[j] = expf(ls);
            const float u = head_row[j] + sd[j] * z[j];
            a[j] = tanhf(u);
            s1 += -(z[j] * z[j]) * 0.5f - ls - 0.9189385332046727f;
            s2 += logf(1.0f - a[j] * a[j] + SAC_EPS);
        }
    }
    return s1 - s2;
}

// the noise of one row: given, or generated from (seed ^ key, row id, draw); written to noise_out where asked
__device__ __forceinline__ void sac_row_noise(const float *__restrict__ noise_in, float *__restrict__ noise_out, int64_t r, int A, uint32_t seed, uint32_t rid,
                                              uint32_t draw, bool deterministic, float (&z)[SAC_MAX_A]) {
#pragma unroll
    for (int j = 0; j < SAC_MAX_A; j++) {
        z[j] = 0.0f;
        if (j < A) {
            z[j] = deterministic ? 0.0f : noise_in ? noise_in[r * A + j] : sac_normal(seed, rid, draw, j);
            if (noise_out) noise_out[r * A + j] = z[j];
        }
    }
}

__device__ __forceinline__ void sac_store_head(float *__restrict__ head_out, const float *head, int64_t row0, int64_t n, int A, int tid) {
    for (int e = tid; e < 16 * 2 * A; e += 256) {
        const int row = e / (2 * A), c = e - row * 2 * A;
        if (row0 + row < n) head_out[(row0 + row) * 2 * A + c] = head[row * DQN_LDQ + (c < A ? c : 8 + c - A)];
    }
}

template <int ACT, int NT>
__global__ __launch_bounds__(256) void sac_act_kernel(const float *__restrict__ actor, SacLayout L, const float *__restrict__ obs, int64_t n, int deterministic,
                                                      uint32_t seed, uint32_t draw, uint32_t row_offset, const float *__restrict__ noise_in,
                                                      float *__restrict__ actions_out, float *__restrict__ logp_out, float *__restrict__ noise_out,
                                                      float *__restrict__ head_out) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], h1[16 * LD], h2[16 * LD], head[16 * DQN_LDQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A;
    const int64_t n_tiles = (n + 15) >> 4;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(obs, row0, n, L.D, X, tid);
        __syncthreads();
        sac_actor_tile<ACT, NT>(actor, L, X, h1, h2, head, lane, wave);
        if (tid < 16 && row0 + tid < n) {
            const int64_t r = row0 + tid;
            float z[SAC_MAX_A], a[SAC_MAX_A], sd[SAC_MAX_A];
            sac_row_noise(noise_in, noise_out, r, A, seed ^ SAC_KEY_COLLECT, row_offset + (uint32_t)r, draw, deterministic != 0, z);
            const float logp = sac_squash_row(head + tid * DQN_LDQ, A, z, a, sd);
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++)
                if (j < A) actions_out[r * A + j] = a[j];
            if (logp_out) logp_out[r] = logp;
        }
        if (head_out) sac_store_head(head_out, head, row0, n, A, tid);
        __syncthreads();  // (the next tile overwrites X and head)
    }
}

// SB3's warm-up below learning_starts: action_space.sample() on [-1, 1)^A, one hash per element, the net is not read
__global__ __launch_bounds__(256) void sac_uniform_kernel(int64_t n, int A, uint32_t seed, uint32_t draw, uint32_t row_offset, float *__restrict__ actions_out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n * A; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / A;
        const int j = (int)(e - r * A);
        actions_out[e] = 2.0f * uniform01(mix32(seed ^ (SAC_KEY_UNIFORM + (uint32_t)j * 0x9E3779B9u), row_offset + (uint32_t)r, draw)) - 1.0f;
    }
}

struct SacCriticArgs {
    const float *actor, *critic, *target, *log_alpha;
    SacLayout L;
    const float *obs, *actions, *next_obs, *dones, *rewards, *discounts, *noise_in;
    int64_t n;
    uint32_t seed, draw;
    float *slabs;    // [grid][2 n_q]
    double *parts;   // [grid][4]: critic-loss sum, sum Q0, sum Q1, rows
    float *q_out, *target_out, *noise_out, *head_out;
};

template <int ACT, int NT>
__global__ __launch_bounds__(256) void sac_critic_kernel(SacCriticArgs a) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], Xn[16 * DQN_LDX], h1[16 * LD], h2[16 * LD], head[16 * DQN_LDQ], qt[32], qv[16], yv[16], lp[16], dz3[16 * DQN_LDQ],
        rowstat[16 * 4];
    const SacLayout &L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A, D = L.D;
    float *slab = a.slabs + (int64_t)blockIdx.x * 2 * L.n_q;
    const float nf = (float)a.n, alpha = expf(a.log_alpha[0]);
    const int64_t n_tiles = (a.n + 15) >> 4;
    TileStats<3> stats;  // thread 0's: critic loss, Q0, Q1
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(a.obs, row0, a.n, D, X, tid);
        dqn_load_tile(a.actions, row0, a.n, A, X + D, tid);  // (obs | a_replay): SB3's concatenation
        dqn_load_tile(a.next_obs, row0, a.n, D, Xn, tid);
        __syncthreads();
        sac_actor_tile<ACT, NT>(a.actor, L, Xn, h1, h2, head, lane, wave);
        if (tid < 16) {
            const int64_t r = row0 + tid;
            float z[SAC_MAX_A], an[SAC_MAX_A], sd[SAC_MAX_A];
            float logp = 0.0f;
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++) an[j] = 0.0f;
            if (r < a.n) {
                sac_row_noise(a.noise_in, a.noise_out, r, A, a.seed ^ SAC_KEY_NEXT, (uint32_t)r, a.draw, false, z);
                logp = sac_squash_row(head + tid * DQN_LDQ, A, z, an, sd);
            }
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++)
                if (j < A) Xn[tid * DQN_LDX + D + j] = an[j];
            lp[tid] = logp;
        }
        if (a.head_out) sac_store_head(a.head_out, head, row0, a.n, A, tid);
        __syncthreads();
        sac_q_tile<ACT, NT>(a.target, L, Xn, h1, h2, qt, lane, wave);
        sac_q_tile<ACT, NT>(a.target + L.n_q, L, Xn, h1, h2, qt + 16, lane, wave);
        if (tid < 16) {
            const int64_t r = row0 + tid;
            float y = 0.0f;
            if (r < a.n) {
                const float m = fminf(qt[tid], qt[16 + tid]) - alpha * lp[tid];
                y = a.rewards[r] + ((1.0f - a.dones[r]) * a.discounts[r]) * m;
                if (a.target_out) a.target_out[r] = y;
            }
            yv[tid] = y;
        }
        __syncthreads();
        for (int i = 0; i < 2; i++) {
            const float *cp = a.critic + (int64_t)i * L.n_q;
            sac_q_tile<ACT, NT>(cp, L, X, h1, h2, qv, lane, wave);
            if (tid < 16) {
                const int64_t r = row0 + tid;
                float ct = 0.0f, loss = 0.0f, q = 0.0f;
                if (r < a.n) {
                    q = qv[tid];
                    const float delta = q - yv[tid];
                    loss = 0.5f * delta * delta;
                    ct = delta / nf;
                    if (a.q_out) a.q_out[r * 2 + i] = q;
                }
                for (int c = 0; c < 16; c++) dz3[tid * DQN_LDQ + c] = c == 0 ? ct : 0.0f;
                rowstat[4 * tid + 2 * i] = loss, rowstat[4 * tid + 2 * i + 1] = q;
            }
            __syncthreads();
            q_backward_tile<ACT, NT>(cp, L, X, h1, h2, dz3, slab + (int64_t)i * L.n_q, first, tid);
            __syncthreads();  // (the next critic / tile overwrites every buffer)
        }
        if (tid == 0) stats.add(row0, a.n, critic_row_stats(rowstat));
        __syncthreads();  // (rowstat is rewritten by the next tile)
        first = false;
    }
    if (tid == 0) stats.store<4>(a.parts);
}

struct SacActorArgs {
    const float *actor, *critic, *log_alpha;
    SacLayout L;
    const float *obs, *noise_in;
    int64_t n;
    uint32_t seed, draw;
    float *slabs;    // [grid][n_actor]
    double *parts;   // [grid][4]: actor-loss sum, sum logp_pi, rows, (unused)
    float *actions_out, *logp_out, *noise_out, *head_out;
};

template <int ACT, int NT>
__global__ __launch_bounds__(256) void sac_actor_kernel(SacActorArgs a) {
    constexpr int H = 64 * NT, LD = H + 2;
    __shared__ float X[16 * DQN_LDX], ha1[16 * LD], ha2[16 * LD], hq1[2][16 * LD], hq2[2][16 * LD], head[16 * DQN_LDQ], dzh[16 * DQN_LDQ], qv[32], dzq[32],
        zs[16 * SAC_MAX_A], ats[16 * SAC_MAX_A], sds[16 * SAC_MAX_A], dA[16 * SAC_MAX_A], rowstat[16 * 2];
    const SacLayout &L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = L.A, D = L.D;
    float *slab = a.slabs + (int64_t)blockIdx.x * L.n_actor;
    const float nf = (float)a.n, alpha = expf(a.log_alpha[0]);
    const int64_t n_tiles = (a.n + 15) >> 4;
    TileStats<2> stats;  // thread 0's: actor loss, logp_pi
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile << 4;
        dqn_load_tile(a.obs, row0, a.n, D, X, tid);
        __syncthreads();
        sac_actor_tile<ACT, NT>(a.actor, L, X, ha1, ha2, head, lane, wave);
        if (tid < 16) {
            const int64_t r = row0 + tid;
            float z[SAC_MAX_A], ap[SAC_MAX_A], sd[SAC_MAX_A];
            float logp = 0.0f;
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++) z[j] = 0.0f, ap[j] = 0.0f, sd[j] = 0.0f;
            if (r < a.n) {
                sac_row_noise(a.noise_in, a.noise_out, r, A, a.seed ^ SAC_KEY_PI, (uint32_t)r, a.draw, false, z);
                logp = sac_squash_row(head + tid * DQN_LDQ, A, z, ap, sd);
#pragma unroll
                for (int j = 0; j < SAC_MAX_A; j++)
                    if (j < A && a.actions_out) a.actions_out[r * A + j] = ap[j];
                if (a.logp_out) a.logp_out[r] = logp;
            }
#pragma unroll
            for (int j = 0; j < SAC_MAX_A; j++) {
                if (j < A) X[tid * DQN_LDX + D + j] = ap[j];
                zs[tid * SAC_MAX_A + j] = z[j], ats[tid * SAC_MAX_A + j] = ap[j], sds[tid * SAC_MAX_A + j] = sd[j];
            }
            rowstat[2 * tid + 1] = logp;
        }
        if (a.head_out) sac_store_head(a.head_out, head, row0, a.n, A, tid);
        __syncthreads();
        sac_q_tile<ACT, NT>(a.critic, L, X, hq1[0], hq2[0], qv, lane, wave);
        sac_q_tile<ACT, NT>(a.critic + L.n_q, L, X, hq1[1], hq2[1], qv + 16, lane, wave);
        if (tid < 16) {  // min(Q0, Q1): on a tie qf0 carries the gradient
            const bool in = row0 + tid < a.n, second = qv[16 + tid] < qv[tid];
            const float ct = in ? -1.0f / nf : 0.0f;
            dzq[tid] = second ? 0.0f : ct, dzq[16 + tid] = second ? ct : 0.0f;
            rowstat[2 * tid] = in ? alpha * rowstat[2 * tid + 1] - (second ? qv[16 + tid] : qv[tid]) : 0.0f;
        }
        __syncthreads();
        if (tid == 0) stats.add_columns(row0, a.n, rowstat);
        q_action_grad_tile<ACT, NT, 2>(a.critic, L, dzq, hq1[0], hq2[0], dA, tid);  // both critics' input gradients down to the action rows of W1
        if (tid < 16) {  // through the squash and logp into the head cotangent
            const bool in = row0 + tid < a.n;
            const float an = alpha / nf;
            for (int c = 0; c < 16; c++) dzh[tid * DQN_LDQ + c] = 0.0f;
            for (int j = 0; j < A && in; j++) {
                const float av = ats[tid * SAC_MAX_A + j], om = 1.0f - av * av;
                const float da = dA[tid * SAC_MAX_A + j] + an * (2.0f * av / (om + SAC_EPS));
                const float du = da * om;
                const float raw = head[tid * DQN_LDQ + 8 + j];
                const float dls = du * sds[tid * SAC_MAX_A + j] * zs[tid * SAC_MAX_A + j] - an;
                dzh[tid * DQN_LDQ + j] = du;
                dzh[tid * DQN_LDQ + 8 + j] = (raw >= SAC_LS_MIN && raw <= SAC_LS_MAX) ? dls : 0.0f;  // torch's clamp passes the gradient inside the bounds
            }
        }
        __syncthreads();
        dqn_wgrad(ha2, LD, H, dzh, DQN_LDQ, A, slab + L.aWmu, first, lane, wave);
        dqn_wgrad(ha2, LD, H, dzh + 8, DQN_LDQ, A, slab + L.aWls, first, lane, wave);
        dqn_bgrad(dzh, DQN_LDQ, A, slab + L.abmu, first, tid);
        dqn_bgrad(dzh + 8, DQN_LDQ, A, slab + L.abls, first, tid);
        __syncthreads();
        for (int e = tid; e < 16 * H; e += 256) {  // ha2 := dz2 = (dmu Wmu^T + dls Wls^T) act'(ha2): mu columns in order, then log_std columns
            const int row = e / H, k = e - row * H;
            float s = 0.0f;
            for (int j = 0; j < A; j++) s += dzh[row * DQN_LDQ + j] * a.actor[L.aWmu + k * A + j];
            for (int j = 0; j < A; j++) s += dzh[row * DQN_LDQ + 8 + j] * a.actor[L.aWls + k * A + j];
            ha2[row * LD + k] = act_bwd<ACT>(s, ha2[row * LD + k]);
        }
        __syncthreads();
        trunk_backward_tile<ACT, NT>(a.actor, slab, L.aW1, L.ab1, L.aW2, L.ab2, X, D, ha1, ha2, first, tid);
        __syncthreads();  // (the next tile overwrites every buffer)
        first = false;
    }
    if (tid == 0) stats.store<4>(a.parts);
}

// d loss / d log_ent_coef of SB3's  -(log_ent_coef * (logp_pi + target_entropy).detach()).mean(), from the float64 sum of logp_pi
__global__ void sac_ent_grad_kernel(const double *__restrict__ actor_stats, double target_entropy, float *__restrict__ grad) {
    if (threadIdx.x == 0 && blockIdx.x == 0) grad[0] = (float)(-(actor_stats[1] / actor_stats[2] + target_entropy));
}

// torch.optim.Adam (no amsgrad, no weight decay) on a flat vector, element-wise in f32 with the IEEE square root and division (AdamRule's arithmetic,
// except that omb1 = 1 - beta1 and omb2 = 1 - beta2 are formed in double on the host and rounded once, as torch passes them)
__global__ __launch_bounds__(256) void sac_adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int64_t n,
                                                       float omb1, float beta2, float omb2, float bc2_sqrt, float eps, float lr_step) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float gv = g[e];
        float mm = m[e], vv = v[e];
        mm = mm + (gv - mm) * omb1;          // exp_avg.lerp_(grad, 1 - beta1)
        vv = vv * beta2 + (gv * gv) * omb2;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        m[e] = mm, v[e] = vv;
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        p[e] = p[e] - lr_step * (mm / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
}

// target <- tau * params + (1 - tau) * target in f32 (two products, one sum, nothing fused); tau == 1: a copy.  THE target update: tma_dqn_target_update runs it too
__global__ __launch_bounds__(256) void polyak_kernel(const float *__restrict__ params, float *__restrict__ target, int64_t n, float tau, float omt, int copy) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float p = params[e];
        target[e] = copy ? p : tau * p + omt * target[e];
    }
}

}  // namespace tma

using namespace tma;

extern "C" {

int tma_sac_param_offsets(const tma_sac_dims *d, tma_sac_offsets *out) {
    const int rc = sac_check(d, "tma_sac_param_offsets");
    if (rc) return rc;
    if (!out) return fail(TMA_ERR_INVALID, "tma_sac_param_offsets: null argument (out)");
    const SacLayout L = sac_layout_of(d);
    out->a_W1 = L.aW1, out->a_b1 = L.ab1, out->a_W2 = L.aW2, out->a_b2 = L.ab2, out->a_Wmu = L.aWmu, out->a_bmu = L.abmu, out->a_Wls = L.aWls, out->a_bls = L.abls;
    out->n_actor = L.n_actor;
    out->q_W1 = L.qW1, out->q_b1 = L.qb1, out->q_W2 = L.qW2, out->q_b2 = L.qb2, out->q_W3 = L.qW3, out->q_b3 = L.qb3;
    out->n_q = L.n_q, out->n_critic = 2 * L.n_q;
    return TMA_OK;
}

int tma_sac_act(const float *actor, const tma_sac_dims *d, const float *obs, int64_t n, int mode, uint32_t seed, uint32_t draw, uint32_t row_offset,
                const float *noise_in, float *actions_out, float *logp_out, float *noise_out, float *head_out, void *stream) {
    int rc = sac_check(d, "tma_sac_act");
    if (rc) return rc;
    if (mode != TMA_SAC_SAMPLE && mode != TMA_SAC_DETERMINISTIC && mode != TMA_SAC_UNIFORM)
        return fail(TMA_ERR_INVALID, "tma_sac_act: mode %d is none of TMA_SAC_SAMPLE (0), TMA_SAC_DETERMINISTIC (1), TMA_SAC_UNIFORM (2)", mode);
    if (!actions_out) return fail(TMA_ERR_INVALID, "tma_sac_act: null argument (actions_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_sac_act: n must be at least 1 (got %lld)", (long long)n);
    const SacLayout L = sac_layout_of(d);
    if (mode == TMA_SAC_UNIFORM) {
        if (noise_in || logp_out || noise_out || head_out)
            return fail(TMA_ERR_INVALID, "tma_sac_act: the uniform mode reads no net and no noise: noise_in, logp_out, noise_out and head_out must be NULL");
        if ((rc = tile_set_device(d->device))) return rc;
        const int64_t nb = ceil_div(n * L.A, 256);
        sac_uniform_kernel<<<dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, (hipStream_t)stream>>>(n, L.A, seed, draw, row_offset, actions_out);
        TMA_LAUNCH_CHECK();
        return TMA_OK;
    }
    if (!actor || !obs) return fail(TMA_ERR_INVALID, "tma_sac_act: null argument (actor or obs)");
    if (mode == TMA_SAC_DETERMINISTIC && noise_in) return fail(TMA_ERR_INVALID, "tma_sac_act: the deterministic mode takes no noise_in");
    if ((rc = tile_set_device(d->device))) return rc;
    const int64_t tiles = (n + 15) >> 4;
    const dim3 grid((unsigned)(tiles < SAC_ACT_GRID_CAP ? tiles : SAC_ACT_GRID_CAP)), block(256);
    TILE_DISPATCH(sac_act_kernel, L, (k<<<grid, block, 0, (hipStream_t)stream>>>(actor, L, obs, n, mode == TMA_SAC_DETERMINISTIC ? 1 : 0, seed, draw, row_offset,
                                                                                 noise_in, actions_out, logp_out, noise_out, head_out)));
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int64_t tma_sac_workspace_bytes(const tma_sac_dims *d, int64_t n) {
    if (sac_check(d, "tma_sac_workspace_bytes")) return 0;
    if (n < 1) {
        fail(TMA_ERR_INVALID, "tma_sac_workspace_bytes: n must be at least 1 (got %lld)", (long long)n);
        return 0;
    }
    return sac_workspace_bytes_of(sac_layout_of(d), n);
}

int tma_sac_critic_grad(const float *actor, const float *critic, const float *critic_target, const float *log_ent_coef, const tma_sac_dims *d, const float *obs,
                        const float *actions, const float *next_obs, const float *dones, const float *rewards, const float *discounts, int64_t n, uint32_t seed,
                        uint32_t draw, const float *noise_in, float *grad_out, double *stats_out, float *q_out, float *target_out, float *noise_out,
                        float *head_out, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = sac_check(d, "tma_sac_critic_grad");
    if (rc) return rc;
    if (!actor || !critic || !critic_target || !log_ent_coef || !obs || !actions || !next_obs || !dones || !rewards || !discounts || !grad_out)
        return fail(TMA_ERR_INVALID,
                    "tma_sac_critic_grad: null argument (actor, critic, critic_target, log_ent_coef, obs, actions, next_obs, dones, rewards, discounts or grad_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_sac_critic_grad: n must be at least 1 (got %lld)", (long long)n);
    const SacLayout L = sac_layout_of(d);
    hipStream_t s = (hipStream_t)stream;
    return sac_grad_run("tma_sac_critic_grad", "tma_sac_workspace_bytes", d, L, n, workspace, workspace_bytes, 2 * L.n_q, 4, grad_out, stats_out, s,
                        [&](int grid, float *slabs, double *parts) {
                            const SacCriticArgs a{actor, critic, critic_target, log_ent_coef, L, obs, actions, next_obs, dones, rewards, discounts,
                                                  noise_in, n, seed, draw, slabs, parts, q_out, target_out, noise_out, head_out};
                            TILE_DISPATCH(sac_critic_kernel, L, (k<<<dim3((unsigned)grid), dim3(256), 0, s>>>(a)));
                        });
}

int tma_sac_actor_grad(const float *actor, const float *critic, const float *log_ent_coef, const tma_sac_dims *d, const float *obs, int64_t n, uint32_t seed,
                       uint32_t draw, const float *noise_in, float *grad_out, double *stats_out, float *actions_out, float *logp_out, float *noise_out,
                       float *head_out, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = sac_check(d, "tma_sac_actor_grad");
    if (rc) return rc;
    if (!actor || !critic || !log_ent_coef || !obs || !grad_out)
        return fail(TMA_ERR_INVALID, "tma_sac_actor_grad: null argument (actor, critic, log_ent_coef, obs or grad_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_sac_actor_grad: n must be at least 1 (got %lld)", (long long)n);
    const SacLayout L = sac_layout_of(d);
    hipStream_t s = (hipStream_t)stream;
    return sac_grad_run("tma_sac_actor_grad", "tma_sac_workspace_bytes", d, L, n, workspace, workspace_bytes, L.n_actor, 3, grad_out, stats_out, s,
                        [&](int grid, float *slabs, double *parts) {
                            const SacActorArgs a{actor, critic, log_ent_coef, L, obs, noise_in, n, seed, draw, slabs, parts, actions_out, logp_out, noise_out, head_out};
                            TILE_DISPATCH(sac_actor_kernel, L, (k<<<dim3((unsigned)grid), dim3(256), 0, s>>>(a)));
                        });
}

int tma_sac_ent_coef_grad(const double *actor_stats, double target_entropy, float *grad_out, void *stream) {
    if (!actor_stats || !grad_out) return fail(TMA_ERR_INVALID, "tma_sac_ent_coef_grad: null argument (actor_stats or grad_out)");
    if (!(target_entropy == target_entropy)) return fail(TMA_ERR_INVALID, "tma_sac_ent_coef_grad: target_entropy is NaN");
    sac_ent_grad_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(actor_stats, target_entropy, grad_out);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int tma_adam_step_flat(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, double lr, double beta1, double beta2,
                       double eps, void *stream) {
    if (!params || !grad || !exp_avg || !exp_avg_sq) return fail(TMA_ERR_INVALID, "tma_adam_step_flat: null argument (params, grad, exp_avg or exp_avg_sq)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_adam_step_flat: n must be at least 1 (got %lld)", (long long)n);
    if (step < 1) return fail(TMA_ERR_INVALID, "tma_adam_step_flat: step must be at least 1 (got %lld)", (long long)step);
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return fail(TMA_ERR_INVALID, "tma_adam_step_flat: lr %g and eps %g must be at least 0, the betas (%g, %g) in [0, 1)", lr, eps, beta1, beta2);
    const AdamArgs args{exp_avg, exp_avg_sq, lr, beta1, beta2, eps, 0.0, 1.0};
    const AdamArgs::Step t = args.at(step);
    const int64_t nb = ceil_div(n, 256);
    sac_adam_kernel<<<dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, (hipStream_t)stream>>>(params, grad, exp_avg, exp_avg_sq, n, (float)(1.0 - beta1),
                                                                                                    (float)beta2, (float)(1.0 - beta2), t.bc2_sqrt, (float)eps,
                                                                                                    t.lr_step);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int tma_polyak_update(const float *params, float *target, int64_t n, double tau, void *stream) {
    if (!params || !target) return fail(TMA_ERR_INVALID, "tma_polyak_update: null argument (params or target)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_polyak_update: n must be at least 1 (got %lld)", (long long)n);
    if (!(tau > 0.0 && tau <= 1.0)) return fail(TMA_ERR_INVALID, "tma_polyak_update: tau %g is outside (0, 1]", tau);
    if (params == target) return fail(TMA_ERR_INVALID, "tma_polyak_update: params and target are the same buffer");
    const int64_t nb = ceil_div(n, 256);
    polyak_kernel<<<dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, (hipStream_t)stream>>>(params, target, n, (float)tau, (float)(1.0 - tau), tau == 1.0 ? 1 : 0);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

int tma_sac_iterations_local(tma_env *env, float *actor, float *critic, float *critic_target, float *log_ent_coef, const tma_sac_dims *d, const tma_replay *rb,
                             const tma_sac_buffers *b, const tma_sac_hparams *hp, tma_sac_counters *c, int n_iters, void *stream) {
    int rc = sac_check(d, "tma_sac_iterations_local");
    if (rc) return rc;
    if (!env || !actor || !critic || !critic_target || !log_ent_coef || !rb || !b || !hp || !c)
        return fail(TMA_ERR_INVALID, "tma_sac_iterations_local: null argument");
    if (!b->last_obs || !b->actions || !b->step_obs || !b->rewards || !b->term || !b->trunc || !b->term_obs || !b->s_obs || !b->s_actions || !b->s_next_obs ||
        !b->s_dones || !b->s_rewards || !b->s_discounts || !b->actor_grad || !b->actor_exp_avg || !b->actor_exp_avg_sq || !b->critic_grad || !b->critic_exp_avg ||
        !b->critic_exp_avg_sq || !b->ent_grad || !b->ent_exp_avg || !b->ent_exp_avg_sq || !b->critic_stats || !b->actor_stats || !b->workspace)
        return fail(TMA_ERR_INVALID, "tma_sac_iterations_local: a buffer of tma_sac_buffers is null");
    if (n_iters < 1) return fail(TMA_ERR_INVALID, "tma_sac_iterations_local: n_iters must be at least 1 (got %d)", n_iters);
    if (hp->train_freq < 1 || hp->batch_size < 1 || hp->target_update_interval < 1 || hp->gradient_steps == 0 || hp->gradient_steps < -1)
        return fail(TMA_ERR_INVALID, "tma_sac_iterations_local: train_freq, batch_size and target_update_interval must be at least 1, gradient_steps >= 1 or -1");
    if (!rb->continuous || rb->obs_dim != d->obs_dim || rb->act_dim != d->act_dim || rb->capacity < 1 || rb->n_envs < 1)
        return fail(TMA_ERR_INVALID, "tma_sac_iterations_local: the replay view must be Box, of the dims' obs_dim and act_dim, with capacity and n_envs >= 1");
    if (c->pos < 0 || c->pos >= rb->capacity || c->num_timesteps < 0 || c->n_calls < 0 || c->adam_step < 0 || c->n_updates < 0)
        return fail(TMA_ERR_INVALID, "tma_sac_iterations_local: counters out of range (pos %lld of %d rows)", (long long)c->pos, rb->capacity);
    const int64_t N = rb->n_envs;
    const int grad_steps = hp->gradient_steps < 0 ? hp->train_freq : hp->gradient_steps;
    const SacLayout L = sac_layout_of(d);
    const int64_t B = hp->batch_size;
    for (int it = 0; it < n_iters; it++) {
        for (int k = 0; k < hp->train_freq; k++) {
            const bool warm = c->num_timesteps < hp->learning_starts;  // SB3's uniform warm-up
            if ((rc = tma_sac_act(warm ? nullptr : actor, d, warm ? nullptr : b->last_obs, N, warm ? TMA_SAC_UNIFORM : TMA_SAC_SAMPLE, hp->rng_seed, c->collect_step,
                                  hp->env_offset, nullptr, b->actions, nullptr, nullptr, nullptr, stream)))
                return rc;
            if ((rc = offpolicy_collect_step(env, rb, b, c, TMA_ACT_F32, stream))) return rc;
        }
        if (c->num_timesteps > hp->learning_starts) {
            for (int gs = 0; gs < grad_steps; gs++) {
                if ((rc = offpolicy_sample(rb, b, hp, c, stream))) return rc;
                const int64_t t = c->adam_step + 1;
                if ((rc = tma_sac_critic_grad(actor, critic, critic_target, log_ent_coef, d, b->s_obs, b->s_actions, b->s_next_obs, b->s_dones, b->s_rewards,
                                              b->s_discounts, B, hp->rng_seed, c->draw, nullptr, b->critic_grad, b->critic_stats, nullptr, nullptr, nullptr, nullptr,
                                              b->workspace, b->workspace_bytes, stream)))
                    return rc;
                if ((rc = tma_adam_step_flat(critic, b->critic_grad, b->critic_exp_avg, b->critic_exp_avg_sq, 2 * (int64_t)L.n_q, t, hp->learning_rate, 0.9, 0.999, 1e-8,
                                             stream)))
                    return rc;
                if ((rc = tma_sac_actor_grad(actor, critic, log_ent_coef, d, b->s_obs, B, hp->rng_seed, c->draw, nullptr, b->actor_grad, b->actor_stats, nullptr, nullptr,
                                             nullptr, nullptr, b->workspace, b->workspace_bytes, stream)))
                    return rc;
                if ((rc = tma_adam_step_flat(actor, b->actor_grad, b->actor_exp_avg, b->actor_exp_avg_sq, L.n_actor, t, hp->learning_rate, 0.9, 0.999, 1e-8, stream)))
                    return rc;
                if (hp->auto_ent_coef) {
                    if ((rc = tma_sac_ent_coef_grad(b->actor_stats, hp->target_entropy, b->ent_grad, stream))) return rc;
                    if ((rc = tma_adam_step_flat(log_ent_coef, b->ent_grad, b->ent_exp_avg, b->ent_exp_avg_sq, 1, t, hp->learning_rate, 0.9, 0.999, 1e-8, stream)))
                        return rc;
                }
                if (c->n_updates % hp->target_update_interval == 0 && (rc = tma_polyak_update(critic, critic_target, 2 * (int64_t)L.n_q, hp->tau, stream))) return rc;
                c->draw += 1;
                c->adam_step += 1;
                c->n_updates += 1;
            }
        }
    }
    return TMA_OK;
}

}  // extern "C"
