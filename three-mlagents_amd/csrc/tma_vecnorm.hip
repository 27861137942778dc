// tma_vecnorm.hip -- SB3's VecNormalize on the device (include/tma.h, ABI 217): running float64 mean / variance of the observations and of the
// per-env discounted returns, normalisation and clipping of observations, rewards and terminal observations.  The device code of a step lives in
// tma_vecnorm.h, which the normalised fused rollout chunks of tma_rollout.hip compile as well; the rollout driver that puts one such step behind
// every env step (tma_rollout_collect_norm) is in tma_rollout.hip, beside the chunk kernels it launches.
//
// State (per handle, HBM, float64): two statistics buffers of 2 D + 4 doubles {mean[D], var[D], obs count, return mean, return var, return
// count} used alternately -- a step reads the current one and writes the other, so no workgroup of a two-launch step can read a value another
// one has already replaced; the host flips the index per updating call -- returns[N], and float32 copies of the last step's raw obs / rewards.
//
// Launch structure.  N <= TMA_VECNORM_ONE_LAUNCH_MAX: ONE workgroup of 256 threads does all six steps of VecNormalize.step_wait.  Larger N:
// vn_moments_kernel (G <= 64 workgroups, each the moments of its own rows) + vn_apply_kernel (every workgroup folds the G partials in index order,
// merges them into the running statistics and normalises its own rows; workgroup 0 stores the new statistics).  Frozen statistics: vn_apply_kernel alone.
//
// Sums: tma_vecnorm.h.  (The column READS of the moments pass have stride D across the lanes of a segment -- uncoalesced at R = 64; the rows were just written by the
// env step and sit in L2.  Staging a block of rows through LDS with row-contiguous loads is the follow-up if the moments pass ever shows up in a
// profile; the STORES of the normalising pass are whole rows by consecutive threads.)
//
// Arithmetic.  -ffp-contract=off -fno-fast-math (csrc/Makefile): the merge and the normalisation are the literal IEEE float64 operation
// sequences of include/tma.h -- subtract, sqrt, divide; no reciprocal square root.
#include "tma_vecnorm.h"

#include <cmath>
#include <new>
#include <vector>

namespace tma {

// LDS: s_mean[D], s_sd[D], part[2 D + 2] (one-launch kernel), s_ret[2], red[4]
__global__ __launch_bounds__(VN_THREADS) void vn_step_one_kernel(VnArgs a) {
    extern __shared__ double vn_lds[];
    const int D = a.D;
    double *s_mean = vn_lds, *s_sd = vn_lds + D, *part = vn_lds + 2 * D, *s_ret = part + 2 * D + 2, *red = s_ret + 2;
    if (a.upd_obs) block_obs_moments(a, 0, a.N, part, part + D);
    if (a.upd_ret) block_ret_moments(a, 0, a.N, part + 2 * D, red);
    __syncthreads();
    fold_and_merge(a, part, s_mean, s_sd, s_ret, true);
    __syncthreads();
    apply_rows(a, 0, a.N, s_mean, s_sd, s_ret[0]);
}

__global__ __launch_bounds__(VN_THREADS) void vn_moments_kernel(VnArgs a) {
    __shared__ double red[4];
    const int g = blockIdx.x, D = a.D;
    const int64_t row0 = (int64_t)g * a.rows_blk, rows = partial_rows(a, g);
    double *part = a.partials + (int64_t)g * (2 * D + 2);
    if (a.upd_obs) block_obs_moments(a, row0, rows, part, part + D);
    if (a.upd_ret) block_ret_moments(a, row0, rows, part + 2 * D, red);
}

__global__ __launch_bounds__(VN_THREADS) void vn_apply_kernel(VnArgs a) {
    extern __shared__ double vn_lds[];
    const int D = a.D;
    double *s_mean = vn_lds, *s_sd = vn_lds + D, *s_ret = vn_lds + 2 * D;
    fold_and_merge(a, a.partials, s_mean, s_sd, s_ret, blockIdx.x == 0);
    __syncthreads();
    const int64_t row0 = (int64_t)blockIdx.x * a.rows_apply;
    int64_t rows = a.N - row0;
    if (rows > a.rows_apply) rows = a.rows_apply;
    if (rows > 0) apply_rows(a, row0, rows, s_mean, s_sd, s_ret[0]);
}

enum { VN_MAP_NORM_OBS = 0, VN_MAP_UNNORM_OBS = 1, VN_MAP_NORM_REW = 2, VN_MAP_UNNORM_REW = 3 };

// stateless maps over `count` floats (rows of D for the observation modes); `on` = 0: a copy
__global__ __launch_bounds__(VN_THREADS) void vn_map_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t count, int D, const double *__restrict__ st,
                                                           int mode, int on, double clip, double eps) {
    const int64_t stride = (int64_t)gridDim.x * VN_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * VN_THREADS + threadIdx.x; e < count; e += stride) {
        const float x = in[e];
        float y = x;
        if (on) {
            if (mode == VN_MAP_NORM_OBS || mode == VN_MAP_UNNORM_OBS) {
                const int d = (int)(e % D);
                const double mean = st[d], sd = sqrt(st[D + d] + eps);
                y = mode == VN_MAP_NORM_OBS ? norm_value(x, mean, sd, clip) : (float)((double)x * sd + mean);
            } else {
                const double sd = sqrt(st[2 * D + 2] + eps);
                y = mode == VN_MAP_NORM_REW ? (float)fmin(fmax((double)x / sd, -clip), clip) : (float)((double)x * sd);
            }
        }
        out[e] = y;
    }
}

int vn_ensure(tma_vecnorm *h) {
    if (h->device >= 0) TMA_HIP(hipSetDevice(h->device));
    if (h->allocated) return TMA_OK;
    const int D = h->D;
    const int64_t N = h->N;
    const size_t stat_bytes = sizeof(double) * (2 * (size_t)D + 4);
    // moments grid: blocks of a multiple of 256 rows, at most VN_MAX_PARTIALS of them
    h->rows_blk = VN_THREADS * ceil_div(N, (int64_t)VN_THREADS * VN_MAX_PARTIALS);
    h->G = (int)ceil_div(N, h->rows_blk);
    TMA_HIP(hipMalloc(&h->stats[0], stat_bytes));
    TMA_HIP(hipMalloc(&h->stats[1], stat_bytes));
    TMA_HIP(hipMalloc(&h->returns, sizeof(double) * (size_t)N));
    TMA_HIP(hipMalloc(&h->partials, sizeof(double) * (size_t)h->G * (2 * (size_t)D + 2)));
    TMA_HIP(hipMalloc(&h->raw_obs, sizeof(float) * (size_t)N * D));
    TMA_HIP(hipMalloc(&h->raw_rew, sizeof(float) * (size_t)N));
    std::vector<double> init(2 * (size_t)D + 4, 0.0);  // RunningMeanStd(epsilon = 1e-4): mean 0, var 1, count 1e-4
    for (int d = 0; d < D; d++) init[D + d] = 1.0;
    init[2 * D] = 1e-4;
    init[2 * D + 2] = 1.0;
    init[2 * D + 3] = 1e-4;
    TMA_HIP(hipMemcpy(h->stats[0], init.data(), stat_bytes, hipMemcpyHostToDevice));
    TMA_HIP(hipMemcpy(h->stats[1], init.data(), stat_bytes, hipMemcpyHostToDevice));
    TMA_HIP(hipMemset(h->returns, 0, sizeof(double) * (size_t)N));
    TMA_HIP(hipMemset(h->partials, 0, sizeof(double) * (size_t)h->G * (2 * (size_t)D + 2)));
    TMA_HIP(hipMemset(h->raw_obs, 0, sizeof(float) * (size_t)N * D));
    TMA_HIP(hipMemset(h->raw_rew, 0, sizeof(float) * (size_t)N));
    TMA_HIP(hipDeviceSynchronize());
    h->cur = 0;
    h->allocated = true;
    return TMA_OK;
}

// one VecNormalize step (rewards == nullptr: the reset form, observations only) on validated arguments
int vn_step(tma_vecnorm *h, float *obs, float *rewards, float *terminal_obs, const uint8_t *terminated, const uint8_t *truncated, int training,
            void *stream) {
    int rc = vn_ensure(h);
    if (rc) return rc;
    const int D = h->D;
    const int64_t N = h->N;
    VnArgs a{};
    a.obs = obs, a.rewards = rewards, a.term_obs = terminal_obs, a.terminated = terminated, a.truncated = truncated;
    a.upd_obs = (training && h->norm_obs) ? 1 : 0;
    a.upd_ret = (training && rewards) ? 1 : 0;
    const bool updates = a.upd_obs || a.upd_ret;
    a.st_in = h->stats[h->cur];
    a.st_out = updates ? h->stats[h->cur ^ 1] : nullptr;
    a.returns = h->returns, a.partials = h->partials, a.raw_obs = h->raw_obs, a.raw_rew = h->raw_rew;
    a.N = N, a.D = D;
    a.norm_obs = h->norm_obs, a.norm_reward = h->norm_reward;
    a.clip_obs = h->clip_obs, a.clip_reward = h->clip_reward, a.gamma = h->gamma, a.eps = h->epsilon;
    hipStream_t s = (hipStream_t)stream;
    if (updates && N <= TMA_VECNORM_ONE_LAUNCH_MAX) {
        a.G = 1, a.rows_blk = N, a.rows_apply = N, a.seg = vn_pow2ceil(N);
        const size_t lds = sizeof(double) * (4 * (size_t)D + 8);
        vn_step_one_kernel<<<dim3(1), dim3(VN_THREADS), lds, s>>>(a);
        TMA_LAUNCH_CHECK();
    } else {
        a.G = h->G, a.rows_blk = h->rows_blk, a.seg = vn_pow2ceil(h->rows_blk);
        if (updates) {
            vn_moments_kernel<<<dim3(a.G), dim3(VN_THREADS), 0, s>>>(a);
            TMA_LAUNCH_CHECK();
        }
        a.rows_apply = VN_THREADS * ceil_div(N, (int64_t)VN_THREADS * VN_MAX_APPLY_BLOCKS);
        const int nb = (int)ceil_div(N, a.rows_apply);
        const size_t lds = sizeof(double) * (2 * (size_t)D + 2);
        vn_apply_kernel<<<dim3(nb), dim3(VN_THREADS), lds, s>>>(a);
        TMA_LAUNCH_CHECK();
    }
    if (updates) h->cur ^= 1;
    return TMA_OK;
}

static int vn_map(tma_vecnorm *h, const char *what, const float *in, float *out, int64_t n, int mode, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "%s: null handle", what);
    if (!in || !out) return fail(TMA_ERR_INVALID, "%s: null plane", what);
    if (n <= 0) return fail(TMA_ERR_INVALID, "%s: n = %lld rows", what, (long long)n);
    int rc = vn_ensure(h);
    if (rc) return rc;
    const bool is_obs = mode == VN_MAP_NORM_OBS || mode == VN_MAP_UNNORM_OBS;
    const int64_t count = is_obs ? n * h->D : n;
    int64_t nb = ceil_div(count, VN_THREADS);
    if (nb > 4096) nb = 4096;
    vn_map_kernel<<<dim3((unsigned)nb), dim3(VN_THREADS), 0, (hipStream_t)stream>>>(in, out, count, h->D, h->stats[h->cur], mode, is_obs ? h->norm_obs : h->norm_reward,
                                                                                    is_obs ? h->clip_obs : h->clip_reward, h->epsilon);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

}  // namespace tma

using namespace tma;

extern "C" int tma_vecnorm_create(int D, int64_t N, int norm_obs, int norm_reward, double clip_obs, double clip_reward, double gamma, double epsilon,
                                  int device, tma_vecnorm **out) {
    if (!out) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: null output pointer");
    *out = nullptr;
    if (D <= 0 || D > TMA_VECNORM_MAX_DIM) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: observation width D = %d (1 .. %d)", D, TMA_VECNORM_MAX_DIM);
    if (N <= 0) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: N = %lld envs", (long long)N);
    if (!(clip_obs > 0.0) || !(clip_reward > 0.0)) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: clip_obs = %g and clip_reward = %g must be positive", clip_obs, clip_reward);
    if (!(epsilon > 0.0)) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: epsilon = %g must be positive", epsilon);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: gamma = %g is outside [0, 1]", gamma);
    tma_vecnorm *h = new (std::nothrow) tma_vecnorm;
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_create: out of host memory");
    h->D = D, h->N = N, h->device = device;
    h->norm_obs = norm_obs ? 1 : 0, h->norm_reward = norm_reward ? 1 : 0;
    h->clip_obs = clip_obs, h->clip_reward = clip_reward, h->gamma = gamma, h->epsilon = epsilon;
    *out = h;
    return TMA_OK;
}

extern "C" int tma_vecnorm_destroy(tma_vecnorm *h) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_destroy: null handle");
    if (h->allocated) {
        if (h->device >= 0) (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(h->stats[0]);
        (void)hipFree(h->stats[1]);
        (void)hipFree(h->returns);
        (void)hipFree(h->partials);
        (void)hipFree(h->raw_obs);
        (void)hipFree(h->raw_rew);
    }
    delete h;
    return TMA_OK;
}

extern "C" int tma_vecnorm_set_flags(tma_vecnorm *h, int norm_obs, int norm_reward) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_set_flags: null handle");
    h->norm_obs = norm_obs ? 1 : 0, h->norm_reward = norm_reward ? 1 : 0;
    return TMA_OK;
}

extern "C" int tma_vecnorm_reset(tma_vecnorm *h, float *obs, int64_t n, int training, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_reset: null handle");
    if (!obs) return fail(TMA_ERR_INVALID, "tma_vecnorm_reset: null observation plane");
    if (n != h->N) return fail(TMA_ERR_INVALID, "tma_vecnorm_reset: %lld rows, the handle has %lld envs", (long long)n, (long long)h->N);
    int rc = vn_ensure(h);
    if (rc) return rc;
    TMA_HIP(hipMemsetAsync(h->returns, 0, sizeof(double) * (size_t)h->N, (hipStream_t)stream));
    return vn_step(h, obs, nullptr, nullptr, nullptr, nullptr, training, stream);
}

extern "C" int tma_vecnorm_step(tma_vecnorm *h, float *obs, float *rewards, float *terminal_obs, const uint8_t *terminated, const uint8_t *truncated,
                                int64_t n, int training, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_step: null handle");
    if (!obs || !rewards || !terminated || !truncated) return fail(TMA_ERR_INVALID, "tma_vecnorm_step: null plane (obs, rewards, terminated and truncated are required)");
    if (n != h->N) return fail(TMA_ERR_INVALID, "tma_vecnorm_step: %lld rows, the handle has %lld envs", (long long)n, (long long)h->N);
    return vn_step(h, obs, rewards, terminal_obs, terminated, truncated, training, stream);
}

extern "C" int tma_vecnorm_normalize_obs(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream) {
    return vn_map(h, "tma_vecnorm_normalize_obs", in, out, n, VN_MAP_NORM_OBS, stream);
}
extern "C" int tma_vecnorm_unnormalize_obs(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream) {
    return vn_map(h, "tma_vecnorm_unnormalize_obs", in, out, n, VN_MAP_UNNORM_OBS, stream);
}
extern "C" int tma_vecnorm_normalize_reward(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream) {
    return vn_map(h, "tma_vecnorm_normalize_reward", in, out, n, VN_MAP_NORM_REW, stream);
}
extern "C" int tma_vecnorm_unnormalize_reward(tma_vecnorm *h, const float *in, float *out, int64_t n, void *stream) {
    return vn_map(h, "tma_vecnorm_unnormalize_reward", in, out, n, VN_MAP_UNNORM_REW, stream);
}

extern "C" int tma_vecnorm_get_stats(tma_vecnorm *h, double *obs_mean_host, double *obs_var_host, double *scalars4_host, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_get_stats: null handle");
    if (!obs_mean_host || !obs_var_host || !scalars4_host) return fail(TMA_ERR_INVALID, "tma_vecnorm_get_stats: null output array");
    int rc = vn_ensure(h);
    if (rc) return rc;
    const int D = h->D;
    std::vector<double> host(2 * (size_t)D + 4);
    TMA_HIP(hipMemcpyAsync(host.data(), h->stats[h->cur], sizeof(double) * host.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    TMA_HIP(hipStreamSynchronize((hipStream_t)stream));
    for (int d = 0; d < D; d++) obs_mean_host[d] = host[d], obs_var_host[d] = host[D + d];
    for (int k = 0; k < 4; k++) scalars4_host[k] = host[2 * D + k];
    return TMA_OK;
}

extern "C" int tma_vecnorm_set_stats(tma_vecnorm *h, const double *obs_mean_host, const double *obs_var_host, const double *scalars4_host, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_set_stats: null handle");
    if (!obs_mean_host || !obs_var_host || !scalars4_host) return fail(TMA_ERR_INVALID, "tma_vecnorm_set_stats: null input array");
    int rc = vn_ensure(h);
    if (rc) return rc;
    const int D = h->D;
    std::vector<double> host(2 * (size_t)D + 4);
    for (int d = 0; d < D; d++) host[d] = obs_mean_host[d], host[D + d] = obs_var_host[d];
    for (int k = 0; k < 4; k++) host[2 * D + k] = scalars4_host[k];
    TMA_HIP(hipMemcpyAsync(h->stats[h->cur], host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    TMA_HIP(hipStreamSynchronize((hipStream_t)stream));
    return TMA_OK;
}

extern "C" int tma_vecnorm_copy_stats(tma_vecnorm *dst, tma_vecnorm *src, void *stream) {
    if (!dst || !src) return fail(TMA_ERR_INVALID, "tma_vecnorm_copy_stats: null handle");
    if (dst->D != src->D) return fail(TMA_ERR_INVALID, "tma_vecnorm_copy_stats: observation widths differ (%d and %d)", dst->D, src->D);
    if (dst == src) return TMA_OK;
    int rc = vn_ensure(src);
    if (rc) return rc;
    rc = vn_ensure(dst);
    if (rc) return rc;
    TMA_HIP(hipMemcpyAsync(dst->stats[dst->cur], src->stats[src->cur], sizeof(double) * (2 * (size_t)src->D + 4), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TMA_OK;
}

extern "C" int tma_vecnorm_get_returns(tma_vecnorm *h, double *returns_host, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_get_returns: null handle");
    if (!returns_host) return fail(TMA_ERR_INVALID, "tma_vecnorm_get_returns: null output array");
    int rc = vn_ensure(h);
    if (rc) return rc;
    TMA_HIP(hipMemcpyAsync(returns_host, h->returns, sizeof(double) * (size_t)h->N, hipMemcpyDeviceToHost, (hipStream_t)stream));
    TMA_HIP(hipStreamSynchronize((hipStream_t)stream));
    return TMA_OK;
}

extern "C" int tma_vecnorm_get_original(tma_vecnorm *h, float *obs_out, float *rewards_out, void *stream) {
    if (!h) return fail(TMA_ERR_INVALID, "tma_vecnorm_get_original: null handle");
    if (!obs_out && !rewards_out) return fail(TMA_ERR_INVALID, "tma_vecnorm_get_original: both outputs are null");
    int rc = vn_ensure(h);
    if (rc) return rc;
    if (obs_out) TMA_HIP(hipMemcpyAsync(obs_out, h->raw_obs, sizeof(float) * (size_t)h->N * h->D, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (rewards_out) TMA_HIP(hipMemcpyAsync(rewards_out, h->raw_rew, sizeof(float) * (size_t)h->N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TMA_OK;
}
