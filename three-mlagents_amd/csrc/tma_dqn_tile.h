// tma_dqn_tile.h -- the tile functions of the four-wave-per-16-row-tile MLP kernels, shared by csrc/tma_dqn.hip and csrc/tma_sac.hip (moved
// here unchanged from tma_dqn.hip).  A workgroup of four waves owns a tile of 16 rows; a hidden layer's H output columns are split over the
// waves (16 NT columns each, NT = H / 64); the tile's activations live in LDS; f32 MFMA (v_mfma_f32_16x16x4_f32) in k order.
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

// rows [row0, row0 + 16) of src f32[n][D] into X[16][DQN_LDX]; rows behind n are zeros
__device__ __forceinline__ void dqn_load_tile(const float *__restrict__ src, int64_t row0, int64_t n, int D, float *X, int tid) {
    for (int e = tid; e < 16 * D; e += 256) {
        const int row = e / D, c = e - row * D;
        X[row * DQN_LDX + c] = row0 + row < n ? src[(row0 + row) * D + c] : 0.0f;
    }
}

}  // namespace tma
