// tma_sac_tile.h -- what csrc/tma_sac.hip and csrc/tma_td3.hip share beyond tma_dqn_tile.h: the flat [in][out] layout of an actor and of a critic
// pair; on a 16-row tile the transposed input gradient of a hidden layer (sac_bwd_input_t), one critic's forward (sac_q_tile), the backward of
// the two hidden layers of an actor or a critic (trunk_backward_tile), one critic's whole backward (q_backward_tile) and the critics' gradient
// with respect to the action (q_action_grad_tile); the Box-Muller noise; the slab fold of a gradient launch; the shape check of tma_sac_dims,
// the workspace size and the frame of a gradient entry (sac_grad_run).  The three backward functions are SAC's two gradient kernels'; TD3's
// kernels spell the same chains out (tma_td3.hip's head says why).  Offsets reach the tile functions by reference: a layout field is then read
// where the layer that needs it runs, as in the text the functions replaced, and the compiler's schedule stays close to that text's.
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
    mlp_trunk_tile<ACT, NT>(X, L.D + L.A, p, L.qW1, L.qb1, L.qW2, L.qb2, h1, h2, lane, wave);
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

// THE backward of a net's two hidden layers, from h2 already holding dz2 (a barrier behind its forming): dW2 / db2, h1 := dz1, dW1 / db1 into the
// block's slab.  oW1 .. ob2 are the layers' offsets, the same in the parameter buffer `p` and in `slab`; X[.][0 .. K) is the net's input.  Every
// thread of the workgroup calls it (it holds barriers); the caller's next barrier stands before any reuse of X, h1, h2.
template <int ACT, int NT>
__device__ __forceinline__ void trunk_backward_tile(const float *p, float *slab, const int &oW1, const int &ob1, const int &oW2, const int &ob2, const float *X,
                                                    int K, float *h1, float *h2, bool first, int tid) {
    constexpr int H = 64 * NT, LD = H + 2;
    const int lane = tid & 63, wave = tid >> 6;
    dqn_wgrad(h1, LD, H, h2, LD, H, slab + oW2, first, lane, wave);
    dqn_bgrad(h2, LD, H, slab + ob2, first, tid);
    __syncthreads();
    sac_bwd_input_t<ACT, NT>(h2, LD, H, p + oW2, h1, LD, lane, wave * 16 * NT);  // h1 := dz1
    __syncthreads();
    dqn_wgrad(X, DQN_LDX, K, h1, LD, H, slab + oW1, first, lane, wave);
    dqn_bgrad(h1, LD, H, slab + ob1, first, tid);
}

// h2 := dz2 = dz3 W3^T act'(h2) of ONE critic, whose head has one column: one product per element.  dz[row * ldz] is the row's head cotangent.
template <int ACT, int NT>
__device__ __forceinline__ void q_head_backward_tile(const float *dz, int ldz, const float *cp, const int &oW3, float *h2, int tid) {
    constexpr int H = 64 * NT, LD = H + 2;
    for (int e = tid; e < 16 * H; e += 256) {
        const int row = e / H, k = e - row * H;
        h2[row * LD + k] = act_bwd<ACT>(dz[row * ldz] * cp[oW3 + k], h2[row * LD + k]);
    }
}

// ONE critic's backward from dz3 (column 0: the head cotangent, visible to every thread) into its slab `sl`: dW3 / db3, h2 := dz2, then
// trunk_backward_tile.  cp is the critic's parameters, X its input tile (obs | action); barriers as trunk_backward_tile.
template <int ACT, int NT>
__device__ __forceinline__ void q_backward_tile(const float *cp, const SacLayout &L, const float *X, float *h1, float *h2, const float *dz3, float *sl, bool first,
                                                int tid) {
    constexpr int H = 64 * NT, LD = H + 2;
    dqn_wgrad(h2, LD, H, dz3, DQN_LDQ, 1, sl + L.qW3, first, tid & 63, tid >> 6);
    dqn_bgrad(dz3, DQN_LDQ, 1, sl + L.qb3, first, tid);
    __syncthreads();
    q_head_backward_tile<ACT, NT>(dz3, DQN_LDQ, cp, L.qW3, h2, tid);
    __syncthreads();
    trunk_backward_tile<ACT, NT>(cp, sl, L.qW1, L.qb1, L.qW2, L.qb2, X, L.D + L.A, h1, h2, first, tid);
}

// a critic kernel's rowstat[16][4] = (loss0, Q0, loss1, Q1) as a row's three statistics for TileStats<3>::add: loss0 + loss1, Q0, Q1
__device__ __forceinline__ auto critic_row_stats(const float *rowstat) {
    return [rowstat](int row, double(&v)[3]) {
        v[0] = (double)rowstat[4 * row] + (double)rowstat[4 * row + 2], v[1] = (double)rowstat[4 * row + 1], v[2] = (double)rowstat[4 * row + 3];
    };
}

// dQ/da of the first NQ critics of `critic`, summed into dA[16][SAC_MAX_A] (no critic weight gradient is formed).  dzq[16 i + row] is critic i's
// head cotangent; hq1 + i 16 LD, hq2 + i 16 LD hold its hidden activations and become dz1, dz2; then thread (row, j) walks the action rows of the
// W1s, h in order, qf0 before qf1.  Every thread of the workgroup calls it; dzq must be visible; on return dA is.
template <int ACT, int NT, int NQ>
__device__ __forceinline__ void q_action_grad_tile(const float *critic, const SacLayout &L, const float *dzq, float *hq1, float *hq2, float *dA, int tid) {
    constexpr int H = 64 * NT, LD = H + 2;
    for (int i = 0; i < NQ; i++) q_head_backward_tile<ACT, NT>(dzq + 16 * i, 1, critic + (int64_t)i * L.n_q, L.qW3, hq2 + i * 16 * LD, tid);
    __syncthreads();
    for (int i = 0; i < NQ; i++)
        sac_bwd_input_t<ACT, NT>(hq2 + i * 16 * LD, LD, H, critic + (int64_t)i * L.n_q + L.qW2, hq1 + i * 16 * LD, LD, tid & 63, (tid >> 6) * 16 * NT);
    __syncthreads();
    const int row = tid >> 4, j = tid & 15;
    if (j < L.A) {
        float s = 0.0f;
        for (int i = 0; i < NQ; i++) {
            const float *w = critic + (int64_t)i * L.n_q + L.qW1 + (int64_t)(L.D + j) * H;
            for (int h = 0; h < H; h++) s += hq1[i * 16 * LD + row * LD + h] * w[h];
        }
        dA[row * SAC_MAX_A + j] = s;
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
static inline SacLayout sac_layout_of(const tma_sac_dims *d) { return sac_layout(d->obs_dim, d->act_dim, d->hidden, d->activation); }

// the workspace of either gradient launch on n rows of layout L (SAC's or TD3's): the blocks' partials, then the wider of the two slab sets
static inline int64_t sac_workspace_bytes_of(const SacLayout &L, int64_t n) {
    const int grid = sac_grad_grid(n);
    const int64_t widest = 2 * (int64_t)L.n_q > L.n_actor ? 2 * (int64_t)L.n_q : L.n_actor;
    return sac_parts_bytes(grid) + (int64_t)grid * widest * 4;
}

// what a gradient entry `who` does around its kernel: refuse a workspace below what `ws_fn` reports, select the device, carve parts and slabs,
// launch(grid, slabs, parts), then fold the slabs of P floats and the first n_stats partials (sac_reduce_kernel)
template <class Launch>
static inline int sac_grad_run(const char *who, const char *ws_fn, const tma_sac_dims *d, const SacLayout &L, int64_t n, void *workspace, int64_t workspace_bytes,
                               int P, int n_stats, float *grad_out, double *stats_out, hipStream_t s, Launch launch) {
    const int64_t need = sac_workspace_bytes_of(L, n);
    if (!workspace || workspace_bytes < need)
        return fail(TMA_ERR_INVALID, "%s: workspace of %lld bytes, %s reports %lld", who, (long long)(workspace ? workspace_bytes : 0), ws_fn, (long long)need);
    const int rc = tile_set_device(d->device);
    if (rc) return rc;
    const int grid = sac_grad_grid(n);
    double *parts = static_cast<double *>(workspace);
    float *slabs = reinterpret_cast<float *>(static_cast<char *>(workspace) + sac_parts_bytes(grid));
    launch(grid, slabs, parts);
    TMA_LAUNCH_CHECK();
    const int rb = (int)ceil_div(P, 256);
    sac_reduce_kernel<<<dim3((unsigned)(rb < 256 ? rb : 256)), dim3(256), 0, s>>>(slabs, parts, grid, P, n_stats, grad_out, stats_out);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

}  // namespace tma
