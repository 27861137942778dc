// tma_dqn_tile.h -- what the off-policy files (csrc/tma_dqn.hip, csrc/tma_sac.hip, csrc/tma_td3.hip) share.
// Device: the tile functions of the four-wave-per-16-row-tile MLP kernels.  A workgroup of four waves owns a tile of 16 rows; a hidden layer's H
// output columns are split over the waves (16 NT columns each, NT = H / 64); the tile's activations live in LDS; f32 MFMA
// (v_mfma_f32_16x16x4_f32) in k order.  dqn_dense / dqn_bwd_input / dqn_wgrad / dqn_bgrad are one layer's pieces, mlp_trunk_tile the two hidden
// layers every forward starts with, TileStats a block's float64 loss sums.
// Host: tile_set_device, the (activation, H) dispatch TILE_DISPATCH, and the two halves of a native iteration that every algorithm issues alike,
// offpolicy_collect_step and offpolicy_sample.
#pragma once
#include "tma_ppo_types.h"

namespace tma {

constexpr int DQN_MAX_OBS = 128;   // obs_dim cap: two [16][DQN_MAX_OBS + 2] tiles beside the activations keep H = 256 below 64 KiB of static LDS
constexpr int DQN_LDX = DQN_MAX_OBS + 2, DQN_LDQ = 17;

// out[16][c0 .. c0 + 16 NT) = act(in[16][K] . Wt[K][N] + b): one wave's share of a hidden layer (dense_act's k order, column by column)
template <int ACT, int NT>
__device__ __forceinline__ void dqn_dense(const float *in, int ldi, int K, const float *__restrict__ Wt, const float *__restrict__ b, int N, float *out,
                                          int ldo, int lane, int c0) {
    const int r16 = lane & 15, g = lane >> 4;
    const int KS = (K + 3) >> 2;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const float bias = b[c0 + 16 * j + r16];
        acc[j] = f32x4{bias, bias, bias, bias};
    }
#pragma unroll 4
    for (int ks = 0; ks < KS; ks++) {
        const int k = 4 * ks + g;
        const bool ok = k < K;
        const float a = ok ? in[r16 * ldi + k] : 0.0f;
        const float *wrow = Wt + (int64_t)(ok ? k : 0) * N + c0 + r16;
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const float w = ok ? wrow[16 * j] : 0.0f;
            acc[j] = mfma16(a, w, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[(g * 4 + r) * ldo + c0 + 16 * j + r16] = act_fwd<ACT>(acc[j][r]);
}

// hbuf[16][c0 .. c0 + 16 NT) = (dzin[16][N] . W[N][K]) * act'(hbuf), IN PLACE: an element is read and then written by the one lane that owns it
template <int ACT, int NT>
__device__ __forceinline__ void dqn_bwd_input(const float *dzin, int ldz, int N, const float *__restrict__ W, int K, float *hbuf, int ldh, int lane, int c0) {
    const int r16 = lane & 15, g = lane >> 4;
    const int NS = (N + 3) >> 2;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int ns = 0; ns < NS; ns++) {
        const int n = 4 * ns + g;
        const bool ok = n < N;
        const float a = ok ? dzin[r16 * ldz + n] : 0.0f;
        const float *wrow = W + (int64_t)(ok ? n : 0) * K + c0 + r16;
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const float w = ok ? wrow[16 * j] : 0.0f;
            acc[j] = mfma16(a, w, acc[j]);
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

// out[K][N] (+)= xin[16][K]^T . dz[16][N]: 16 x 16 output tiles dealt to the four waves in turn; `first`: store, else load-add-store
__device__ __forceinline__ void dqn_wgrad(const float *xin, int ldx, int K, const float *dz, int ldz, int N, float *__restrict__ out, bool first, int lane,
                                          int wave) {
    const int r16 = lane & 15, g = lane >> 4;
    const int kt = (K + 15) >> 4, nt = (N + 15) >> 4;
    for (int t = wave; t < kt * nt; t += 4) {
        const int k0 = (t / nt) << 4, n0 = (t % nt) << 4;
        const int krow = k0 + r16, col = n0 + r16;
        f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const float a = krow < K ? xin[(4 * s + g) * ldx + krow] : 0.0f;
            const float bv = col < N ? dz[(4 * s + g) * ldz + col] : 0.0f;
            acc = mfma16(a, bv, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int k = k0 + g * 4 + r;
            if (k < K && col < N) {
                float *d = out + (int64_t)k * N + col;
                *d = first ? acc[r] : *d + acc[r];
            }
        }
    }
}
// out[N] (+)= column sums of dz[16][N], rows in order
__device__ __forceinline__ void dqn_bgrad(const float *dz, int ldz, int N, float *__restrict__ out, bool first, int tid) {
    for (int c = tid; c < N; c += 256) {
        float s = dz[c];
#pragma unroll
        for (int row = 1; row < 16; row++) s += dz[row * ldz + c];
        out[c] = first ? s : out[c] + s;
    }
}

// THE two hidden layers of every off-policy net: h1 = act(X[.][0 .. K) W1 + b1), h2 = act(h1 W2 + b2), a barrier behind each; oW1 .. ob2 are the
// layers' offsets in the parameter buffer `p` (a layer's address is formed where the layer runs, as before the function existed: the compiler's
// schedule follows it).  Every thread of the workgroup calls it; X must be complete (a barrier behind its load); on return h1, h2 are visible.
template <int ACT, int NT>
__device__ __forceinline__ void mlp_trunk_tile(const float *X, int K, const float *p, const int &oW1, const int &ob1, const int &oW2, const int &ob2,
                                               float *h1, float *h2, int lane, int wave) {
    constexpr int H = 64 * NT, LD = H + 2;
    dqn_dense<ACT, NT>(X, DQN_LDX, K, p + oW1, p + ob1, H, h1, LD, lane, wave * 16 * NT);
    __syncthreads();
    dqn_dense<ACT, NT>(h1, LD, H, p + oW2, p + ob2, H, h2, LD, lane, wave * 16 * NT);
    __syncthreads();
}

// rows [row0, row0 + 16) of src f32[n][D] into X[16][DQN_LDX]; rows behind n are zeros
__device__ __forceinline__ void dqn_load_tile(const float *__restrict__ src, int64_t row0, int64_t n, int D, float *X, int tid) {
    for (int e = tid; e < 16 * D; e += 256) {
        const int row = e / D, c = e - row * D;
        X[row * DQN_LDX + c] = row0 + row < n ? src[(row0 + row) * D + c] : 0.0f;
    }
}

// thread 0's float64 sums of a gradient kernel's block: NS statistics and the rows counted
template <int NS>
struct TileStats {
    double s[NS] = {}, rows = 0.0;
    // one tile: row_stats(row, v) gives the NS values of a row; the tile's valid rows are added in order
    template <class F>
    __device__ __forceinline__ void add(int64_t row0, int64_t n, F row_stats) {
        for (int row = 0; row < 16 && row0 + row < n; row++) {
            double v[NS];
            row_stats(row, v);
#pragma unroll
            for (int k = 0; k < NS; k++) s[k] += v[k];
            rows += 1.0;
        }
    }
    // ... where a row's values are the columns of rowstat[16][NS]
    __device__ __forceinline__ void add_columns(int64_t row0, int64_t n, const float *rowstat) {
        add(row0, n, [rowstat](int row, double(&v)[NS]) {
#pragma unroll
            for (int k = 0; k < NS; k++) v[k] = (double)rowstat[NS * row + k];
        });
    }
    // the block's W partials: the sums, the rows, zeros behind them
    template <int W>
    __device__ __forceinline__ void store(double *__restrict__ parts) const {
        double *p = parts + W * (int64_t)blockIdx.x;
#pragma unroll
        for (int k = 0; k < NS; k++) p[k] = s[k];
        p[NS] = rows;
#pragma unroll
        for (int k = NS + 1; k < W; k++) p[k] = 0.0;
    }
};

static inline int tile_set_device(int device) {
    if (device >= 0) {
        int cur = -1;
        TMA_HIP(hipGetDevice(&cur));
        if (cur != device) TMA_HIP(hipSetDevice(device));
    }
    return TMA_OK;
}

// ONE vector step of a native iteration behind the algorithm's own act call: the envs step on b->actions, the transition goes into the ring at
// c->pos, the counters move on.  (Buffers, Counters: tma_{dqn,sac,td3}_{buffers,counters}, whose field names agree.)
template <class Buffers, class Counters>
static inline int offpolicy_collect_step(tma_env *env, const tma_replay *rb, const Buffers *b, Counters *c, int action_kind, void *stream) {
    int rc;
    if ((rc = tma_env_step(env, b->actions, action_kind, 0, 0, 1, b->step_obs, b->rewards, b->term, b->trunc, b->term_obs, nullptr, nullptr, stream))) return rc;
    if ((rc = tma_replay_add(rb, c->pos, b->last_obs, b->actions, b->step_obs, b->rewards, b->term, b->trunc, b->term_obs, stream))) return rc;
    c->collect_step += 1;
    c->pos += 1;
    if (c->pos == rb->capacity) c->pos = 0, c->full = 1;
    c->num_timesteps += rb->n_envs;
    c->n_calls += 1;
    return TMA_OK;
}

// the minibatch of one optimizer step, drawn with c->draw into the s_* buffers (c->draw is the caller's to bump)
template <class Buffers, class HParams, class Counters>
static inline int offpolicy_sample(const tma_replay *rb, const Buffers *b, const HParams *hp, const Counters *c, void *stream) {
    const int size = c->full ? rb->capacity : (int)c->pos;
    const int newest = (int)((c->pos + rb->capacity - 1) % rb->capacity);
    return tma_replay_sample(rb, size, newest, hp->n_step, hp->gamma, hp->sample_seed, c->draw, hp->batch_size, b->s_obs, b->s_actions, b->s_next_obs, b->s_dones,
                             b->s_rewards, b->s_discounts, nullptr, nullptr, stream);
}

}  // namespace tma

// f(kernel template instance) for (activation, H)
#define TILE_DISPATCH(KERNEL, L, CALL)                                            \
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
