// tma_sac_tile.h -- what csrc/tma_sac.hip and csrc/tma_td3.hip share (moved here unchanged from tma_sac.hip): the flat [in][out] layout of an
// actor and of a critic pair, the transposed input gradient of a hidden layer, one critic's forward on a 16-row tile, the Box-Muller noise, the
// slab fold of a gradient launch, the shape check of tma_sac_dims and the (activation, H) dispatch.
#pragma once
#include "tma_dqn_tile.h"

namespace tma {

constexpr int SAC_GRID_CAP = 64;       // workgroups of a gradient kernel at the most (= slabs in the workspace); more tiles are walked with this stride
constexpr int SAC_ACT_GRID_CAP = 1024;
constexpr int SAC_MAX_A = 8;           // mu in columns [0, 8), log_std in columns [8, 16) of ONE 16-column head tile

struct SacLayout {
    int D, A, H, act;
    int aW1, ab1, aW2, ab2, aWmu, abmu, aWls, abls, n_actor;  // the actor buffer
    int qW1, qb1, qW2, qb2, qW3, qb3, n_q;                    // ONE critic; qf1 follows qf0 at n_q
};
__host__ __device__ inline SacLayout sac_layout(int D, int A, int H, int act) {
    SacLayout L;
    L.D = D, L.A = A, L.H = H, L.act = act;
    int o = 0;
    L.aW1 = o, o += D * H;
    L.ab1 = o, o += H;
    L.aW2 = o, o += H * H;
    L.ab2 = o, o += H;
    L.aWmu = o, o += H * A;
    L.abmu = o, o += A;
    L.aWls = o, o += H * A;
    L.abls = o, o += A;
    L.n_actor = o;
    o = 0;
    L.qW1 = o, o += (D + A) * H;
    L.qb1 = o, o += H;
    L.qW2 = o, o += H * H;
    L.qb2 = o, o += H;
    L.qW3 = o, o += H;
    L.qb3 = o, o += 1;
    L.n_q = o;
    return L;
}

// hbuf[16][c0 .. c0 + 16 NT) = (dz[16][N] . Wt[K][N]^T) * act'(hbuf), IN PLACE, from the [in][out] matrix (row stride N, N % 16 == 0): for a block
// of 16 reduction indices lane group g takes n = 16 blk + 4 g + s at MFMA step s, so a lane reads four consecutive dwords of ITS row of Wt
template <int ACT, int NT>
__device__ __forceinline__ void sac_bwd_input_t(const float *dz, int ldz, int N, const float *__restrict__ Wt, float *hbuf, int ldh, int lane, int c0) {
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int nb = 0; nb < N; nb += 16) {
        float w[NT][4];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const float *wrow = Wt + (int64_t)(c0 + 16 * j + r16) * N + nb + 4 * g;
#pragma unroll
            for (int s = 0; s < 4; s++) w[j][s] = wrow[s];
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const float a = dz[r16 * ldz + nb + 4 * g + s];
#pragma unroll
            for (int j = 0; j < NT; j++) acc[j] = mfma16(a, w[j][s], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float *h = hbuf + (g * 4 + r) * ldh + c0 + 16 * j + r16;
            *h = act_bwd<ACT>(acc[j][r], *h);
        }
}

// ONE critic's forward on X[.][0 .. D + A): q[16]; h1, h2 keep the hidden activations.  Every thread of the workgroup calls it (it holds
// barriers); X must be complete; on return q, h1, h2 are visible to every thread.
template <int ACT, int NT>
__device__ __forceinline__ void sac_q_tile(const float *__restrict__ p, const SacLayout &L, const float *X, float *h1, float *h2, float *q, int lane, int wave) {
    constexpr int H = 64 * NT, LD = H + 2;
    dqn_dense<ACT, NT>(X, DQN_LDX, L.D + L.A, p + L.qW1, p + L.qb1, H, h1, LD, lane, wave * 16 * NT);
    __syncthreads();
    dqn_dense<ACT, NT>(h1, LD, H, p + L.qW2, p + L.qb2, H, h2, LD, lane, wave * 16 * NT);
    __syncthreads();
    if (wave == 0) {
        f32x4 acc[1];
        dense_head<1>(h2, LD, H, p + L.qW3, p + L.qb3, 1, acc, lane);
        const int r16 = lane & 15, g = lane >> 4;
        if (r16 == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++) q[g * 4 + r] = acc[0][r];
        }
    }
    __syncthreads();
}

// z of (stream key, row id, draw, column): Box-Muller on the hardware units, tma_policy.hip's sampler
__device__ __forceinline__ float sac_normal(uint32_t seed, uint32_t rid, uint32_t draw, int col) {
    const float u1 = fmaxf(uniform01(mix32(seed ^ (0x68E31DA4u + (uint32_t)col * 0x9E3779B9u), rid, draw)), 5.9604645e-08f);
    const float u2 = uniform01(mix32(seed ^ (0xB5297A4Du + (uint32_t)col * 0x85EBCA77u), rid, draw));
    return __builtin_amdgcn_sqrtf(-2.0f * __logf(u1)) * __builtin_amdgcn_cosf(u2);
}

// grad[e] = slab_0[e] + slab_1[e] + ... in block order; thread 0 folds the blocks' float64 partials (four per block) in block order
// (static: each translation unit that includes this header launches its own copy)
static __global__ __launch_bounds__(256) void sac_reduce_kernel(const float *__restrict__ slabs, const double *__restrict__ parts, int nb, int P, int n_stats,
                                                                float *__restrict__ grad, double *__restrict__ stats) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < P; e += gridDim.x * 256) {
        float s = slabs[e];
        for (int b = 1; b < nb; b++) s += slabs[(int64_t)b * P + e];
        grad[e] = s;
    }
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
        for (int k = 0; k < n_stats; k++) {
            double s = parts[k];
            for (int b = 1; b < nb; b++) s += parts[4 * b + k];
            stats[k] = s;
        }
    }
}

static inline int sac_grad_grid(int64_t n) {
    const int64_t tiles = (n + 15) >> 4;
    return (int)(tiles < SAC_GRID_CAP ? tiles : SAC_GRID_CAP);
}
static inline int64_t sac_parts_bytes(int grid) { return (int64_t)grid * 4 * 8; }

// the shapes tma_sac_* and tma_td3_* take: every refusal before any HIP call
static inline int sac_check(const tma_sac_dims *d, const char *who) {
    if (!d) return fail(TMA_ERR_INVALID, "%s: null argument (dims)", who);
    if (d->hidden != 64 && d->hidden != 128 && d->hidden != 256) return fail(TMA_ERR_INVALID, "%s: hidden %d is not one of 64, 128, 256", who, d->hidden);
    if (d->act_dim < 1 || d->act_dim > SAC_MAX_A)
        return fail(TMA_ERR_INVALID, "%s: act_dim %d is outside [1, %d] (mu and log_std share one 16-column head tile)", who, d->act_dim, SAC_MAX_A);
    if (d->obs_dim < 1 || d->obs_dim + d->act_dim > DQN_MAX_OBS)
        return fail(TMA_ERR_INVALID, "%s: obs_dim %d + act_dim %d is outside [2, %d] (the critic's input tile)", who, d->obs_dim, d->act_dim, DQN_MAX_OBS);
    if (d->activation != TMA_ACT_TANH && d->activation != TMA_ACT_RELU)
        return fail(TMA_ERR_INVALID, "%s: activation %d is neither TMA_ACT_TANH (0) nor TMA_ACT_RELU (1)", who, d->activation);
    return TMA_OK;
}
static inline int sac_set_device(const tma_sac_dims *d) {
    if (d->device >= 0) {
        int cur = -1;
        TMA_HIP(hipGetDevice(&cur));
        if (cur != d->device) TMA_HIP(hipSetDevice(d->device));
    }
    return TMA_OK;
}
static inline SacLayout sac_layout_of(const tma_sac_dims *d) { return sac_layout(d->obs_dim, d->act_dim, d->hidden, d->activation); }

}  // namespace tma

// f(kernel template instance) for (activation, H)
#define SAC_DISPATCH(KERNEL, L, CALL)                                             \
    do {                                                                          \
        if ((L).act == ACT_RELU) {                                                \
            if ((L).H == 64) { auto k = KERNEL<ACT_RELU, 1>; CALL; }              \
            else if ((L).H == 128) { auto k = KERNEL<ACT_RELU, 2>; CALL; }        \
            else { auto k = KERNEL<ACT_RELU, 4>; CALL; }                          \
        } else {                                                                  \
            if ((L).H == 64) { auto k = KERNEL<ACT_TANH, 1>; CALL; }              \
            else if ((L).H == 128) { auto k = KERNEL<ACT_TANH, 2>; CALL; }        \
            else { auto k = KERNEL<ACT_TANH, 4>; CALL; }                          \
        }                                                                         \
    } while (0)
