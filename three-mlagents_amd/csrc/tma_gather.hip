// tma_gather.hip -- tma_rollout_gather (ABI 221): one minibatch of SB3's RolloutBuffer.get as dense device tensors.
// The gradient kernels of tma_policy.hip / tma_h64.hip / tma_bf16.hip gather their rows themselves and never form a minibatch in memory; a
// caller who writes the update in torch (a loss on evaluate_actions / get_distribution, tma_vjp.hip) needs the rows.  This is the same row
// selection -- sample_offset (tma_ppo_types.h): mb->indices or perm_index, env-major flat index f = i*T + t read from plane row t*N + i --
// as a pure copy: no arithmetic on the data, no atomics, no workspace.
//
// Shape of the kernel.  The output of a minibatch is contiguous, the source rows are scattered: the STORE side is kept fully coalesced and the
// loads are whatever the permutation makes them (whole rows of D floats, so at least row-granular).  A wave owns a block of `rpw` (16 or 64)
// consecutive output rows.  Lane l < rpw evaluates the permutation for row l once and copies that row's scalars (old value, old log-prob,
// advantage, return, a Discrete action) lane-per-row: coalesced stores, gathered loads.  The wave then walks the block's rows x D observation
// floats (and the rows x A floats of Box actions) lane-linearly; the source row of an element comes from its owning lane by a cross-lane read
// (ds_bpermute).  Rows of 21 / 45 / 105 / 172 floats are not 16-byte aligned, so the walk moves dwords unless the row width is a multiple of
// four floats and both bases are 16-byte aligned, where it moves float4.
// The grid is capped at GATHER_BLOCKS workgroups (tma_workspace.h) and strides over the row blocks.  Every offset is 64-bit: T*N*D*4 passes
// 2^32 bytes at the benchmark shapes; T*N itself is below 2^31 (checked), so a row's plane offset travels between lanes as one int.
#include "tma_gather_rows.h"
#include "tma_ppo_types.h"

namespace tma {

struct GatherArgs {
    const float *obs;         // [T][N][D]
    const void *actions;      // i32 [T][N] | f32 [T][N][A]
    const float *values, *log_probs, *advantages, *returns;  // [T][N]
    float *obs_out;           // [count][D]
    void *actions_out;        // i32 [count] | f32 [count][A]
    float *values_out, *log_probs_out, *advantages_out, *returns_out;  // [count]
    int T, D, A, cont, rpw;   // rpw: rows per wave block, 16 or 64
    int64_t N;
};

template <int VEC>
__global__ __launch_bounds__(64 * GATHER_WAVES) void rollout_gather_kernel(GatherArgs g, Minibatch mb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_blocks = (mb.count + g.rpw - 1) / g.rpw;
    for (int64_t blk = (int64_t)blockIdx.x * GATHER_WAVES + wave; blk < n_blocks; blk += (int64_t)gridDim.x * GATHER_WAVES) {
        const int64_t j0 = blk * g.rpw;  // first row of the block inside the minibatch
        const int rows = (int)(mb.count - j0 < g.rpw ? mb.count - j0 : g.rpw);
        int off = 0;
        if (lane < rows) {
            off = (int)sample_offset(mb, mb.start + j0 + lane, g.T, g.N);
            const int64_t j = j0 + lane;
            if (g.values_out) g.values_out[j] = g.values[off];
            if (g.log_probs_out) g.log_probs_out[j] = g.log_probs[off];
            if (g.advantages_out) g.advantages_out[j] = g.advantages[off];
            if (g.returns_out) g.returns_out[j] = g.returns[off];
            if (g.actions_out && !g.cont) static_cast<int32_t *>(g.actions_out)[j] = static_cast<const int32_t *>(g.actions)[off];
        }
        if (g.obs_out) {
            if constexpr (VEC == 4)
                gather_rows(reinterpret_cast<const float4 *>(g.obs), reinterpret_cast<float4 *>(g.obs_out) + j0 * (g.D / 4), off, rows, g.D / 4, lane);
            else
                gather_rows(g.obs, g.obs_out + j0 * g.D, off, rows, g.D, lane);
        }
        if (g.actions_out && g.cont)
            gather_rows(static_cast<const float *>(g.actions), static_cast<float *>(g.actions_out) + j0 * g.A, off, rows, g.A, lane);
    }
}

}  // namespace tma

using namespace tma;

extern "C" int tma_rollout_gather(const tma_rollout *rb, const float *values, const tma_policy_dims *d, const tma_minibatch *mb, float *obs_out,
                                  void *actions_out, float *old_values_out, float *old_log_prob_out, float *advantages_out, float *returns_out,
                                  void *stream) {
    // every refusal comes back before the first HIP call
    if (!rb || !d || !mb) return fail(TMA_ERR_INVALID, "tma_rollout_gather: null argument (rollout view, policy dims or minibatch)");
    int rc = tma_check_policy_dims(d);
    if (rc) return rc;
    if (rb->T < 1 || rb->N < 1) return fail(TMA_ERR_INVALID, "tma_rollout_gather: rollout view needs T >= 1 and N >= 1 (got %d, %lld)", rb->T, (long long)rb->N);
    if (rb->N >= (1ll << 31) || (int64_t)rb->T * rb->N >= (1ll << 31))
        return fail(TMA_ERR_INVALID, "tma_rollout_gather: T * N must be below 2^31 (got %d x %lld)", rb->T, (long long)rb->N);
    const int64_t total = (int64_t)rb->T * rb->N;
    if (old_values_out && !values) return fail(TMA_ERR_INVALID, "tma_rollout_gather: old_values_out given without a values plane");
    if ((obs_out && !rb->obs) || (actions_out && !rb->actions) || (old_log_prob_out && !rb->log_probs) || (advantages_out && !rb->advantages) ||
        (returns_out && !rb->returns))
        return fail(TMA_ERR_INVALID, "tma_rollout_gather: an output was asked for whose source plane is null");
    if (mb->count < 1 || mb->start < 0 || mb->start > total || mb->count > total - mb->start)
        return fail(TMA_ERR_INVALID, "tma_rollout_gather: rows [%lld, %lld + %lld) are not inside the %lld samples of the rollout", (long long)mb->start,
                    (long long)mb->start, (long long)mb->count, (long long)total);
    if (d->device >= 0) {
        int cur = -1;
        TMA_HIP(hipGetDevice(&cur));
        if (cur != d->device) TMA_HIP(hipSetDevice(d->device));
    }
    GatherArgs g{rb->obs, rb->actions, values, rb->log_probs, rb->advantages, rb->returns, obs_out, actions_out, old_values_out, old_log_prob_out,
                 advantages_out, returns_out, rb->T, d->obs_dim, d->act_dim, d->continuous ? 1 : 0, 0, rb->N};
    // 16-row blocks where a block is still several wave-wide stores (four times as many waves for the latency of the gathered loads), else 64
    g.rpw = d->obs_dim >= 16 ? 16 : 64;
    const Minibatch M{mb->indices, mb->perm_seed, mb->perm_epoch, mb->start, mb->count, total, nullptr, mb->count, nullptr, 0};
    const int64_t wg = ceil_div(ceil_div(mb->count, g.rpw), GATHER_WAVES);
    const dim3 grid((unsigned)(wg < GATHER_BLOCKS ? wg : GATHER_BLOCKS)), block(64 * GATHER_WAVES);
    const bool vec4 = d->obs_dim % 4 == 0 && (((uintptr_t)rb->obs | (uintptr_t)obs_out) & 15) == 0;
    if (vec4) rollout_gather_kernel<4><<<grid, block, 0, (hipStream_t)stream>>>(g, M);
    else rollout_gather_kernel<1><<<grid, block, 0, (hipStream_t)stream>>>(g, M);
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}
