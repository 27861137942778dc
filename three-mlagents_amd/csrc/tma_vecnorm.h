// tma_vecnorm.h -- the VecNormalize handle and the device code of one VecNormalize step, shared by tma_vecnorm.hip (the one-launch, moments and
// apply kernels) and tma_rollout.hip (the normalised fused rollout chunks): both translation units compile THESE functions, so a fused chunk
// gets its bits from the code the one-launch kernel runs, in its summation order.  Everything here assumes a 256-thread workgroup; the whole
// library is built with -ffp-contract=off -fno-fast-math (csrc/Makefile), which this code depends on.
//
// Sums.  Column d of a workgroup's rows is summed by a segment of R = min(64, pow2ceil(rows)) lanes of one wave: lane l adds rows l, l + R, ...
// in order, then a __shfl_down tree of width R; two passes (mean, then squared distances from it).  The returns have one row per thread: wave
// tree, four wave partials through LDS, added in wave order.  Workgroup partials (rows, mean, M2) are combined by Chan's formula in index order.
// Nothing depends on anything but (N, D): no atomics, the same bits on every run.
#pragma once
#include "tma_internal.h"

struct tma_vecnorm {
    int D = 0, device = -1;
    int64_t N = 0;
    int norm_obs = 1, norm_reward = 1;
    double clip_obs = 10.0, clip_reward = 10.0, gamma = 0.99, epsilon = 1e-8;
    // device memory, allocated on first use
    bool allocated = false;
    double *stats[2] = {nullptr, nullptr};  // [2 D + 4] each
    int cur = 0;
    double *returns = nullptr;   // [N]
    double *partials = nullptr;  // [G][2 D + 2]: column means, column M2s, return mean, return M2 of workgroup g's rows
    float *raw_obs = nullptr, *raw_rew = nullptr;
    int G = 1;                   // workgroups of vn_moments_kernel
    int64_t rows_blk = 0;        // rows of each (the last one: what is left)
};

namespace tma {

constexpr int VN_THREADS = 256, VN_MAX_PARTIALS = 64, VN_MAX_APPLY_BLOCKS = 1024;

struct VnArgs {
    float *obs, *rewards, *term_obs;
    const uint8_t *terminated, *truncated;
    const double *st_in;
    double *st_out;  // nullptr: frozen statistics
    double *returns, *partials;
    float *raw_obs, *raw_rew;
    int64_t N, rows_blk, rows_apply;
    int D, G, seg;
    int upd_obs, upd_ret, norm_obs, norm_reward;
    double clip_obs, clip_reward, gamma, eps;
};

// segment width of the column sums over `n` rows
inline int vn_pow2ceil(int64_t n) {
    int p = 1;
    while (p < n && p < 64) p <<= 1;
    return p;
}

// tma_vecnorm.hip: device memory of a handle on its first use; one VecNormalize step (rewards == nullptr: the reset form, observations only) on
// validated arguments
int vn_ensure(tma_vecnorm *h);
int vn_step(tma_vecnorm *h, float *obs, float *rewards, float *terminal_obs, const uint8_t *terminated, const uint8_t *truncated, int training, void *stream);

// sum over a segment of R consecutive lanes (R a power of two <= 64), left in every lane of the segment
__device__ __forceinline__ double seg_sum(double v, int R) {
    for (int o = R >> 1; o > 0; o >>= 1) v += __shfl_down(v, o, R);
    return __shfl(v, 0, R);
}

// sum over the workgroup's 256 threads: wave tree, four partials through LDS, added in wave order; left in every thread
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();  // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// column means and M2s (sums of squared distances from the mean) of rows [row0, row0 + rows)
static __device__ void block_obs_moments(const VnArgs &a, int64_t row0, int64_t rows, double *out_mean, double *out_m2) {
    const int R = a.seg, S = VN_THREADS / R, seg = threadIdx.x / R, lr = threadIdx.x % R, D = a.D;
    const float *x = a.obs + row0 * D;
    for (int d0 = 0; d0 < D; d0 += S) {
        const int d = d0 + seg;
        const bool ok = d < D;
        double s = 0.0;
        if (ok)
            for (int64_t r = lr; r < rows; r += R) s += (double)x[r * D + d];
        s = seg_sum(s, R);
        const double m = s / (double)rows;
        double q = 0.0;
        if (ok)
            for (int64_t r = lr; r < rows; r += R) {
                const double c = (double)x[r * D + d] - m;
                q += c * c;
            }
        q = seg_sum(q, R);
        if (ok && lr == 0) {
            out_mean[d] = m;
            out_m2[d] = q;
        }
    }
}

// returns = returns * gamma + rewards over rows [row0, row0 + rows), stored; their mean and M2 into out2
static __device__ void block_ret_moments(const VnArgs &a, int64_t row0, int64_t rows, double *out2, double *red) {
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += VN_THREADS) {
        const double v = a.returns[row0 + r] * a.gamma + (double)a.rewards[row0 + r];
        a.returns[row0 + r] = v;
        s += v;
    }
    const double m = block_sum(s, red) / (double)rows;
    double q = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += VN_THREADS) {  // (each thread re-reads what it stored itself)
        const double c = a.returns[row0 + r] - m;
        q += c * c;
    }
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
        out2[0] = m;
        out2[1] = q;
    }
}

__device__ __forceinline__ int64_t partial_rows(const VnArgs &a, int g) {
    const int64_t left = a.N - (int64_t)g * a.rows_blk;
    return left < a.rows_blk ? left : a.rows_blk;
}

// Chan's combination of the G partials of one quantity in index order: batch mean and population variance over the N rows
__device__ __forceinline__ void fold_partials(const VnArgs &a, const double *part, int stride, int off_mean, int off_m2, double &bm, double &bv) {
    double n = (double)partial_rows(a, 0), mean = part[off_mean], m2 = part[off_m2];
    for (int g = 1; g < a.G; g++) {
        const double nb = (double)partial_rows(a, g), mb = part[(int64_t)g * stride + off_mean], qb = part[(int64_t)g * stride + off_m2];
        const double delta = mb - mean, tot = n + nb;
        mean = mean + delta * nb / tot;
        m2 = m2 + qb + delta * delta * n * nb / tot;
        n = tot;
    }
    bm = mean;
    bv = m2 / (double)a.N;
}

// RunningMeanStd.update_from_moments: the operation sequence of include/tma.h
__device__ __forceinline__ void rms_merge(double mean, double var, double count, double bm, double bv, double n, double &new_mean, double &new_var) {
    const double delta = bm - mean;
    const double tot = count + n;
    new_mean = mean + delta * n / tot;
    const double m_a = var * count;
    const double m_b = bv * n;
    const double M2 = m_a + m_b + delta * delta * count * n / tot;
    new_var = M2 / tot;
}

// New statistics from the partials (or the current ones where nothing updates): column mean and sqrt(var + eps) into LDS, the return's
// sqrt(var + eps) into s_ret[0]; `store`: this workgroup also writes the statistics buffer of the next step.
static __device__ void fold_and_merge(const VnArgs &a, const double *part, double *s_mean, double *s_sd, double *s_ret, bool store) {
    const int D = a.D, stride = 2 * D + 2;
    const double *in = a.st_in;
    const double n = (double)a.N;
    for (int d = threadIdx.x; d < D; d += VN_THREADS) {
        double nm = in[d], nv = in[D + d];
        if (a.upd_obs) {
            double bm, bv;
            fold_partials(a, part, stride, d, D + d, bm, bv);
            rms_merge(in[d], in[D + d], in[2 * D], bm, bv, n, nm, nv);
        }
        s_mean[d] = nm;
        s_sd[d] = sqrt(nv + a.eps);
        if (store && a.st_out) {
            a.st_out[d] = nm;
            a.st_out[D + d] = nv;
        }
    }
    if (threadIdx.x == 0) {
        double rm = in[2 * D + 1], rv = in[2 * D + 2];
        if (a.upd_ret) {
            double bm, bv;
            fold_partials(a, part, stride, 2 * D, 2 * D + 1, bm, bv);
            rms_merge(in[2 * D + 1], in[2 * D + 2], in[2 * D + 3], bm, bv, n, rm, rv);
        }
        s_ret[0] = sqrt(rv + a.eps);
        if (store && a.st_out) {
            a.st_out[2 * D] = a.upd_obs ? in[2 * D] + n : in[2 * D];
            a.st_out[2 * D + 1] = rm;
            a.st_out[2 * D + 2] = rv;
            a.st_out[2 * D + 3] = a.upd_ret ? in[2 * D + 3] + n : in[2 * D + 3];
        }
    }
}

__device__ __forceinline__ float norm_value(float x, double mean, double sd, double clip) {
    const double y = ((double)x - mean) / sd;
    return (float)fmin(fmax(y, -clip), clip);
}

// steps 2, 4, 5, 6 on rows [row0, row0 + rows): whole rows of D floats are read and stored by consecutive threads.  `tile` (a fused rollout
// chunk's LDS observation rows [rows][ldt], else nullptr) also takes every normalised observation: the next step's layer 1 reads it there.
static __device__ void apply_rows(const VnArgs &a, int64_t row0, int64_t rows, const double *s_mean, const double *s_sd, double ret_sd, float *tile = nullptr,
                                  int ldt = 0) {
    const int D = a.D;
    const int64_t base = row0 * D, count = rows * D;
    for (int64_t e = threadIdx.x; e < count; e += VN_THREADS) {
        const int d = (int)(e % D);
        const float x = a.obs[base + e];
        if (a.raw_obs) a.raw_obs[base + e] = x;
        if (a.norm_obs) {
            const float y = norm_value(x, s_mean[d], s_sd[d], a.clip_obs);
            a.obs[base + e] = y;
            if (tile) tile[(e / D) * ldt + d] = y;
        }
    }
    if (a.term_obs && a.norm_obs && a.terminated) {
        for (int64_t e = threadIdx.x; e < count; e += VN_THREADS) {
            const int64_t row = row0 + e / D;
            if (a.terminated[row] | a.truncated[row]) {
                const int d = (int)(e % D);
                a.term_obs[base + e] = norm_value(a.term_obs[base + e], s_mean[d], s_sd[d], a.clip_obs);
            }
        }
    }
    if (a.rewards) {
        for (int64_t r = threadIdx.x; r < rows; r += VN_THREADS) {
            const int64_t i = row0 + r;
            const float x = a.rewards[i];
            if (a.raw_rew) a.raw_rew[i] = x;
            if (a.norm_reward) a.rewards[i] = (float)fmin(fmax((double)x / ret_sd, -a.clip_reward), a.clip_reward);
            if (a.terminated[i] | a.truncated[i]) a.returns[i] = 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------
// A VecNormalize step inside a fused rollout chunk (tma_rollout.hip, the NORM forms of the 8-env-tile f32 kernels).  The kernel is a
// 256-thread workgroup that owns rows [row0, row0 + rows) of the vector; after its env step has stored the raw next observations, rewards,
// flags and terminal observations of those rows, and behind a __syncthreads(), it runs vn_chunk_step on them: the body of vn_step_one_kernel
// (training: the workgroup owns the WHOLE vector, row0 = 0 and rows = N, G = 1) or of vn_apply_kernel (frozen statistics: any tile).
// The running statistics stay in LDS as doubles for the whole chunk, in two buffers used alternately exactly as the handle's two are.
// ------------------------------------------------------------------------------------------
struct VnChunk {
    VnArgs a;                // the handle's flags, constants, returns and raw copies; N, G = 1, rows_blk = N, seg; the kernel sets the planes per step
    const double *stats_in;  // the handle's current statistics
    double *stats_out;       // where the chunk leaves the new ones; nullptr: frozen statistics
};
struct VnNone {};  // (the kernel argument of the un-normalised instantiations)

// doubles of LDS: two statistics buffers [2 D + 4], s_mean[D], s_sd[D], part[2 D + 2], s_ret[2], red[4]
constexpr int vn_chunk_lds_doubles(int D) { return 2 * (2 * D + 4) + 2 * D + (2 * D + 2) + 2 + 4; }

struct VnChunkLds {
    double *st0, *s_mean, *s_sd, *part, *s_ret, *red;
    int st_len;
    __device__ __forceinline__ VnChunkLds(double *base, int D) {
        st0 = base, st_len = 2 * D + 4, s_mean = st0 + 2 * st_len, s_sd = s_mean + D, part = s_sd + D, s_ret = part + 2 * D + 2, red = s_ret + 2;
    }
    __device__ __forceinline__ double *st(int p) const { return st0 + p * st_len; }
};

// before the step loop (the caller's next __syncthreads() publishes it): training -- the statistics into LDS buffer 0; frozen -- the column
// means, sqrt(var + eps) and the return's, once for the whole chunk
static __device__ void vn_chunk_begin(const VnChunk &c, const VnChunkLds &l) {
    if (c.stats_out) {
        for (int e = threadIdx.x; e < 2 * c.a.D + 4; e += VN_THREADS) l.st(0)[e] = c.stats_in[e];
    } else {
        VnArgs a = c.a;
        a.st_in = c.stats_in, a.st_out = nullptr;
        fold_and_merge(a, nullptr, l.s_mean, l.s_sd, l.s_ret, false);
    }
}

// one step; `a` carries this step's planes; p: the LDS statistics buffer that is current (flipped by an updating step)
static __device__ void vn_chunk_step(VnArgs &a, const VnChunkLds &l, bool updates, int &p, int64_t row0, int64_t rows, float *tile, int ldt) {
    if (updates) {
        a.st_in = l.st(p), a.st_out = l.st(p ^ 1);
        if (a.upd_obs) block_obs_moments(a, row0, rows, l.part, l.part + a.D);
        if (a.upd_ret) block_ret_moments(a, row0, rows, l.part + 2 * a.D, l.red);
        __syncthreads();
        fold_and_merge(a, l.part, l.s_mean, l.s_sd, l.s_ret, true);
        __syncthreads();
        p ^= 1;
    }
    apply_rows(a, row0, rows, l.s_mean, l.s_sd, l.s_ret[0], tile, ldt);
}

// after the step loop (behind the step's closing __syncthreads()): the new statistics to the handle's other buffer
static __device__ void vn_chunk_end(const VnChunk &c, const VnChunkLds &l, int p) {
    if (c.stats_out)
        for (int e = threadIdx.x; e < 2 * c.a.D + 4; e += VN_THREADS) c.stats_out[e] = l.st(p)[e];
}

}  // namespace tma
