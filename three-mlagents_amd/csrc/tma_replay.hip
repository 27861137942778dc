// tma_replay.hip -- SB3's ReplayBuffer / NStepReplayBuffer on the device (ABI 224): tma_replay_add, tma_replay_sample, tma_egreedy_actions.
// The off-policy counterpart of tma_gather.hip.  The storage is the caller's (struct tma_replay, include/tma.h); the ring position and the fill
// state are call arguments the host keeps.  Three kernels, one launch per call, no atomics, no workspace, nothing synchronises; every plane
// offset is 64-bit, every grid is capped and strides.
//
// add: an element-wise pass over the N x D floats of a vector step.  Element e of env i = e / D goes to obs[pos] from last_obs, to
// next_obs[pos] from term_obs where the env's step ended its episode and from step_obs elsewhere, and step_obs[e] becomes the new last_obs[e]
// (read and written by the one thread that owns e).  The first N (Box: N x A) threads copy the scalars as well.
//
// sample: the shape of rollout_gather_kernel.  A wave owns a block of 16 or 64 output rows; lane l draws (t, i) for row l, walks its n-step
// window (reward sum in float64, in k order) and stores the row's scalars lane-per-row; the wave then copies the rows' observations, next
// observations and Box actions with gather_rows (tma_gather_rows.h): stores coalesced, float4 only where the row width and all four bases allow.
//
// egreedy: a thread per row of q[n][A], A <= 16.
#include "tma_gather_rows.h"
#include "tma_workspace.h"

namespace tma {

constexpr uint32_t REPLAY_ENV_KEY = 0x5EEDBA5Eu;   // seed ^ this: the env draw of tma_replay_sample
constexpr uint32_t EGREEDY_PICK_KEY = 0xE9517EEDu;  // rng_seed ^ this: the random action of tma_egreedy_actions
constexpr int REPLAY_MAX_N_STEP = 64, REPLAY_MAX_WIDTH = 4096;  // (gather_rows: a block's elements, 64 * width, stay exact in f32)

struct ReplayAddArgs {
    tma_replay rb;
    int64_t pos;
    float *last_obs;
    const void *actions;
    const float *step_obs, *rewards, *term_obs;
    const uint8_t *term, *trunc;
};

__global__ __launch_bounds__(256) void replay_add_kernel(ReplayAddArgs a) {
    const int64_t N = a.rb.n_envs, D = a.rb.obs_dim, A = a.rb.continuous ? a.rb.act_dim : 1;
    const int64_t nd = N * D, na = N * A, n = nd > na ? nd : na, row = a.pos * N;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < nd) {
            const int64_t i = (e >> 32) ? e / D : (int64_t)((uint32_t)e / (uint32_t)D);
            const float stepped = a.step_obs[e];
            const bool ended = a.term_obs && (a.term[i] | a.trunc[i]);
            a.rb.obs[row * D + e] = a.last_obs[e];
            a.rb.next_obs[row * D + e] = ended ? a.term_obs[e] : stepped;
            a.last_obs[e] = stepped;
        }
        if (e < na) {
            if (a.rb.continuous) static_cast<float *>(a.rb.actions)[row * A + e] = static_cast<const float *>(a.actions)[e];
            else static_cast<int32_t *>(a.rb.actions)[row + e] = static_cast<const int32_t *>(a.actions)[e];
        }
        if (e < N) {
            a.rb.rewards[row + e] = a.rewards[e];
            a.rb.terminated[row + e] = a.term[e];
            a.rb.truncated[row + e] = a.trunc[e];
        }
    }
}

struct ReplaySampleArgs {
    tma_replay rb;
    int size, newest, n_step, rpw;  // rpw: rows per wave block, 16 or 64
    double gamma;
    uint32_t seed, draw;
    int64_t count;
    float *obs_out, *next_obs_out, *dones_out, *rewards_out, *discounts_out;
    void *actions_out;
    int32_t *rows_out, *envs_out;
};

template <int VEC>
__global__ __launch_bounds__(64 * GATHER_WAVES) void replay_sample_kernel(ReplaySampleArgs s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = s.rb.capacity, N = (int)s.rb.n_envs, D = s.rb.obs_dim, A = s.rb.act_dim;
    const int64_t n_blocks = (s.count + s.rpw - 1) / s.rpw;
    for (int64_t blk = (int64_t)blockIdx.x * GATHER_WAVES + wave; blk < n_blocks; blk += (int64_t)gridDim.x * GATHER_WAVES) {
        const int64_t j0 = blk * s.rpw;
        const int rows = (int)(s.count - j0 < s.rpw ? s.count - j0 : s.rpw);
        int off = 0, off_last = 0;  // plane rows t*N + i of the first and of the last included step (R*N < 2^31, checked)
        if (lane < rows) {
            const int64_t j = j0 + lane;
            const uint32_t b = (uint32_t)j;
            const int t = (int)(((uint64_t)mix32(s.seed, b, s.draw) * (uint64_t)s.size) >> 32);
            const int i = (int)(mix32(s.seed ^ REPLAY_ENV_KEY, b, s.draw) % (uint32_t)N);
            off = off_last = t * N + i;
            // the n-step window: rows t, t+1, ... (mod R) while k < n_step, ending behind a step that ended its episode and behind row `newest`
            double acc = (double)s.rb.rewards[off], g = s.gamma;
            int row = t;
            for (int k = 1; k < s.n_step; k++) {
                if ((s.rb.terminated[off_last] | s.rb.truncated[off_last]) || row == s.newest) break;
                row = row + 1 == R ? 0 : row + 1;
                off_last = row * N + i;
                acc += g * (double)s.rb.rewards[off_last];
                g *= s.gamma;
            }
            if (s.rewards_out) s.rewards_out[j] = (float)acc;
            if (s.discounts_out) s.discounts_out[j] = (float)g;
            if (s.dones_out) s.dones_out[j] = s.rb.terminated[off_last] ? 1.0f : 0.0f;
            if (s.rows_out) s.rows_out[j] = t;
            if (s.envs_out) s.envs_out[j] = i;
            if (s.actions_out && !s.rb.continuous) static_cast<int32_t *>(s.actions_out)[j] = static_cast<const int32_t *>(s.rb.actions)[off];
        }
        if constexpr (VEC == 4) {
            if (s.obs_out) gather_rows(reinterpret_cast<const float4 *>(s.rb.obs), reinterpret_cast<float4 *>(s.obs_out) + j0 * (D / 4), off, rows, D / 4, lane);
            if (s.next_obs_out)
                gather_rows(reinterpret_cast<const float4 *>(s.rb.next_obs), reinterpret_cast<float4 *>(s.next_obs_out) + j0 * (D / 4), off_last, rows, D / 4, lane);
        } else {
            if (s.obs_out) gather_rows(static_cast<const float *>(s.rb.obs), s.obs_out + j0 * D, off, rows, D, lane);
            if (s.next_obs_out) gather_rows(static_cast<const float *>(s.rb.next_obs), s.next_obs_out + j0 * D, off_last, rows, D, lane);
        }
        if (s.actions_out && s.rb.continuous)
            gather_rows(static_cast<const float *>(s.rb.actions), static_cast<float *>(s.actions_out) + j0 * A, off, rows, A, lane);
    }
}

__global__ __launch_bounds__(256) void egreedy_kernel(const float *__restrict__ q, int64_t n, int A, float eps, uint32_t rng_seed, uint32_t rng_step,
                                                      uint32_t env_offset, int32_t *__restrict__ actions_out) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t env = env_offset + (uint32_t)r;
        int a = 0;
        if (uniform01(mix32(rng_seed, env, rng_step)) < eps) {
            a = (int)(mix32(rng_seed ^ EGREEDY_PICK_KEY, env, rng_step) % (uint32_t)A);
        } else {  // the first maximal column; a NaN never wins, a row of NaNs gives 0
            float m = q[r * A];
            for (int c = 1; c < A; c++) {
                const float v = q[r * A + c];
                if (v > m || (m != m && v == v)) m = v, a = c;
            }
        }
        actions_out[r] = a;
    }
}

// the geometry every entry checks; the planes `need_planes` asks for must all be there
static int check_replay(const char *who, const tma_replay *rb, bool need_planes) {
    if (!rb) return fail(TMA_ERR_INVALID, "%s: null argument (replay view)", who);
    if (rb->capacity < 1 || rb->n_envs < 1) return fail(TMA_ERR_INVALID, "%s: replay view needs capacity >= 1 and n_envs >= 1 (got %d, %lld)", who, rb->capacity, (long long)rb->n_envs);
    if (rb->obs_dim < 1 || rb->obs_dim > REPLAY_MAX_WIDTH || rb->act_dim < 1 || rb->act_dim > REPLAY_MAX_WIDTH)
        return fail(TMA_ERR_INVALID, "%s: obs_dim and act_dim must be in [1, %d] (got %d, %d)", who, REPLAY_MAX_WIDTH, rb->obs_dim, rb->act_dim);
    if (need_planes && (!rb->obs || !rb->next_obs || !rb->actions || !rb->rewards || !rb->terminated || !rb->truncated))
        return fail(TMA_ERR_INVALID, "%s: a plane of the replay view is null", who);
    return TMA_OK;
}

}  // namespace tma

using namespace tma;

extern "C" int tma_replay_add(const tma_replay *rb, int64_t pos, float *last_obs_inout, const void *actions, const float *step_obs, const float *rewards,
                              const uint8_t *term, const uint8_t *trunc, const float *term_obs, void *stream) {
    // every refusal comes back before the first HIP call
    int rc = check_replay("tma_replay_add", rb, true);
    if (rc) return rc;
    if (!last_obs_inout || !actions || !step_obs || !rewards || !term || !trunc)
        return fail(TMA_ERR_INVALID, "tma_replay_add: null argument (last_obs_inout, actions, step_obs, rewards, term or trunc)");
    if (pos < 0 || pos >= rb->capacity) return fail(TMA_ERR_INVALID, "tma_replay_add: pos %lld is outside [0, %d)", (long long)pos, rb->capacity);
    const int64_t nd = rb->n_envs * rb->obs_dim;
    const uintptr_t lo = (uintptr_t)last_obs_inout, so = (uintptr_t)step_obs, bytes = (uintptr_t)nd * sizeof(float);
    if (lo < so + bytes && so < lo + bytes) return fail(TMA_ERR_INVALID, "tma_replay_add: last_obs_inout overlaps step_obs");
    const int64_t na = rb->n_envs * (rb->continuous ? rb->act_dim : 1);
    const int64_t wg = ceil_div(nd > na ? nd : na, 256);
    replay_add_kernel<<<dim3((unsigned)(wg < GATHER_BLOCKS ? wg : GATHER_BLOCKS)), dim3(256), 0, (hipStream_t)stream>>>(
        ReplayAddArgs{*rb, pos, last_obs_inout, actions, step_obs, rewards, term_obs, term, trunc});
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

extern "C" int tma_replay_sample(const tma_replay *rb, int size, int newest, int n_step, double gamma, uint32_t seed, uint32_t draw, int64_t count,
                                 float *obs_out, void *actions_out, float *next_obs_out, float *dones_out, float *rewards_out, float *discounts_out,
                                 int32_t *rows_out, int32_t *envs_out, void *stream) {
    // every refusal comes back before the first HIP call
    int rc = check_replay("tma_replay_sample", rb, false);
    if (rc) return rc;
    if (rb->n_envs >= (1ll << 31) || (int64_t)rb->capacity * rb->n_envs >= (1ll << 31))
        return fail(TMA_ERR_INVALID, "tma_replay_sample: capacity * n_envs must be below 2^31 (got %d x %lld)", rb->capacity, (long long)rb->n_envs);
    if (size < 1 || size > rb->capacity) return fail(TMA_ERR_INVALID, "tma_replay_sample: size %d is outside [1, capacity %d]", size, rb->capacity);
    if (newest < 0 || newest >= size) return fail(TMA_ERR_INVALID, "tma_replay_sample: newest %d is outside the %d valid rows", newest, size);
    if (count < 1) return fail(TMA_ERR_INVALID, "tma_replay_sample: count must be at least 1 (got %lld)", (long long)count);
    if (n_step < 1 || n_step > REPLAY_MAX_N_STEP) return fail(TMA_ERR_INVALID, "tma_replay_sample: n_step %d is outside [1, %d]", n_step, REPLAY_MAX_N_STEP);
    if (!obs_out && !actions_out && !next_obs_out && !dones_out && !rewards_out && !discounts_out && !rows_out && !envs_out)
        return fail(TMA_ERR_INVALID, "tma_replay_sample: every output is null");
    // the draw's window walk reads the rewards and both flag planes whatever is asked for; the three wide planes only behind their outputs
    if (!rb->rewards || !rb->terminated || !rb->truncated || (obs_out && !rb->obs) || (actions_out && !rb->actions) || (next_obs_out && !rb->next_obs))
        return fail(TMA_ERR_INVALID, "tma_replay_sample: a source plane is null (rewards, terminated, truncated, or the plane of an output that was asked for)");
    ReplaySampleArgs s{*rb, size, newest, n_step, 0, gamma, seed, draw, count, obs_out, next_obs_out, dones_out, rewards_out, discounts_out, actions_out,
                       rows_out, envs_out};
    s.rpw = rb->obs_dim >= 16 ? 16 : 64;
    const int64_t wg = ceil_div(ceil_div(count, s.rpw), GATHER_WAVES);
    const dim3 grid((unsigned)(wg < GATHER_BLOCKS ? wg : GATHER_BLOCKS)), block(64 * GATHER_WAVES);
    const uintptr_t bases = (obs_out ? (uintptr_t)rb->obs | (uintptr_t)obs_out : 0) | (next_obs_out ? (uintptr_t)rb->next_obs | (uintptr_t)next_obs_out : 0);
    if (rb->obs_dim % 4 == 0 && (bases & 15) == 0) replay_sample_kernel<4><<<grid, block, 0, (hipStream_t)stream>>>(s);
    else replay_sample_kernel<1><<<grid, block, 0, (hipStream_t)stream>>>(s);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}

extern "C" int tma_egreedy_actions(const float *q, int64_t n, int A, double eps, uint32_t rng_seed, uint32_t rng_step, uint32_t env_offset,
                                   int32_t *actions_out, void *stream) {
    if (!q || !actions_out) return fail(TMA_ERR_INVALID, "tma_egreedy_actions: null argument (q or actions_out)");
    if (n < 1) return fail(TMA_ERR_INVALID, "tma_egreedy_actions: n must be at least 1 (got %lld)", (long long)n);
    if (A < 2 || A > 16) return fail(TMA_ERR_INVALID, "tma_egreedy_actions: A %d is outside [2, 16]", A);
    if (!(eps >= 0.0 && eps <= 1.0)) return fail(TMA_ERR_INVALID, "tma_egreedy_actions: eps %g is outside [0, 1]", eps);
    const int64_t wg = ceil_div(n, 256);
    egreedy_kernel<<<dim3((unsigned)(wg < GATHER_BLOCKS ? wg : GATHER_BLOCKS)), dim3(256), 0, (hipStream_t)stream>>>(q, n, A, (float)eps, rng_seed, rng_step,
                                                                                                                  env_offset, actions_out);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}
