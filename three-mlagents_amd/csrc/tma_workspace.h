// tma_workspace.h -- where everything lives in the update workspace (tma_ppo_workspace_bytes): the ONE definition every translation unit of
// the PPO / A2C update takes its pointers from (host side).  DESIGN.md section 4.1 is the map: size, writers and readers of each region.
//   fixed header | slabs | sample offsets | epoch advantage partials | wide sum-of-squares slots | dz1 cache | (16-byte aligned) fold state
// Two regions OVERLAY the slab area and are live only while no gradient launch uses the slabs they cover:
//   persist_region()  from the slab base: scratch of the persistent epoch kernels (tma_h64p.hip / tma_h256p.hip), which use no slabs
//   defer_w2()        from slab DEFER_W2_SLAB: dW2 deferral buffer of the eight-wave f32 wide kernel, planned only at <= 64 slabs
#pragma once
#include "tma_mlp.h"
#include <cassert>

namespace tma {

constexpr int MAX_GRAD_BLOCKS = 2048;  // rows of 8 doubles in the statistic slots
constexpr int H64_BLOCKS = 128;        // block PAIRS (policy block + value block): 256 blocks = one per CU, a single round
constexpr int BF_SLABS = 160;          // column-parallel kernels: up to 160 policy-net blocks (+ value-net blocks sharing the first slabs)
constexpr int64_t OFFS_CAP = 1 << 22;  // sample offsets cached behind the slabs (int32 each): an epoch, or several of a persistent launch
constexpr int64_t EPOCH_PART_BYTES = ((OFFS_CAP / 1024) + (OFFS_CAP / 256)) * 16;  // advantage partials of every minibatch of an epoch
constexpr int WIDE_SQ_SLOTS = 8192;    // sum-of-squares partials of slab_reduce_kernel for policies beyond the 256 slots of the header
constexpr int64_t DZ1_CAP = 1 << 18;   // samples per minibatch whose dz1 images fit the workspace cache (two-pass layouts only)
constexpr int W2_DEFER_ROWS = 1024;    // rows per image of the dW2 deferral buffer ([net][h1 | dz2][W2_DEFER_ROWS][H]: half-group minibatches of <= 1024 samples)
constexpr int ADV_BLOCKS = 128;        // partial blocks per minibatch at the most (1 024 rows each up to 131 072 rows, longer slices beyond)
constexpr int GATHER_BLOCKS = 2048;    // workgroups of tma_rollout_gather at the most (four waves each: 32 waves a CU), then it strides (uses no workspace)

// (round 6: ... and 97 .. 128 observations with a Box head at H = 256 -- Ant-v5's 105 -- as four layer-1 k-steps)
static inline bool bf_two_pass(const PLayout &L) {
    return L.bf16 && ((L.D > 32 && L.D <= 64) || (L.D > 160 && L.D <= 192) || (L.D > 96 && L.D <= 128 && L.cont && L.H == 256));
}
// (round 6: ... and 97 .. 112 observations -- the reference's ant task, Ant-v5's 105 -- with Box heads at H = 256: seven k-tiles)
static inline bool f32_two_pass(const PLayout &L) {
    return !L.bf16 && L.fr_pi >= 0 && ((L.D > 160 && L.D <= 176) || (L.D > 96 && L.D <= 112 && L.cont && L.H == 256));
}
// the 256-wide layouts tma_h256p.hip takes
static inline bool h256p_layout(const PLayout &L) { return !L.bf16 && L.fr_pi >= 0 && L.H == 256 && !L.cont && L.A <= 16 && L.D <= 32; }
static inline int slab_cap(const PLayout &L) { return (L.bf16 || L.fr_pi >= 0) ? BF_SLABS : H64_BLOCKS; }  // partial-gradient slabs in the workspace

// The fixed header and what starts at the slab base: all a caller without the policy's shape can address.
struct WorkspaceHeader {
    static constexpr int64_t ADV = 0, NORM_PART = 64, NORM_OUT = 64 + 256 * 8, PERSIST_ERR = 2176, PERSIST_FALLBACKS = PERSIST_ERR + 8, PERSIST_SNAP = 2560,
                             ADV_PART = 4096, STATS = 8192, STATS_BYTES = (int64_t)MAX_GRAD_BLOCKS * 8 * 8, SNAP_BYTES = 8 * 8 * 8, BYTES = STATS + STATS_BYTES;
    char *base;
    explicit WorkspaceHeader(void *ws) : base(static_cast<char *>(ws)) {}
    template <class T> T *at(int64_t off) const { return reinterpret_cast<T *>(base + off); }

    float *adv() const { return at<float>(ADV); }                          // [2] minibatch advantage mean, std
    double *norm_partials() const { return at<double>(NORM_PART); }        // [256] gradient sum-of-squares partials
    double *norm_out() const { return at<double>(NORM_OUT); }              // [2] total gradient norm, clip coefficient
    int *persist_err() const { return at<int>(PERSIST_ERR); }              // set when a persistent epoch kernel gave up on a wait
    long long *persist_fallbacks() const { return at<long long>(PERSIST_FALLBACKS); }  // epochs handed back to the per-minibatch launches
    double *persist_stats_snap() const { return at<double>(PERSIST_SNAP); }  // [8][8] statistic slots before a persistent launch (SNAP_BYTES)
    double *adv_partials() const { return at<double>(ADV_PART); }          // [ADV_BLOCKS][2] (sum, sumsq) of a minibatch outside a prepared epoch
    double *stats() const { return at<double>(STATS); }                    // [MAX_GRAD_BLOCKS][8] loss statistic slots (STATS_BYTES)
    float *slabs() const { return at<float>(BYTES); }                      // [slab_cap][P] partial-gradient slabs
    char *persist_region() const { return base + BYTES; }                  // OVERLAYS the slabs: persistent epoch kernels only
};

struct Workspace : WorkspaceHeader {
    static constexpr int DEFER_W2_SLAB = 64;
    static int64_t slab_bytes(const PLayout &L) { return (int64_t)slab_cap(L) * L.P * 4; }
    static int64_t defer_w2_floats(const PLayout &L) { return 2 * (int64_t)2 * W2_DEFER_ROWS * L.H; }  // both nets' [h1 | dz2] pairs
    static bool defer_w2_fits(const PLayout &L) { return ((int64_t)DEFER_W2_SLAB * L.P + defer_w2_floats(L)) * 4 <= slab_bytes(L); }
    static int64_t dz1_cache_bytes(const PLayout &L) {  // both nets; bf16 images or f32 MFMA operands
        return bf_two_pass(L) ? 2 * DZ1_CAP * L.H * 2 : (f32_two_pass(L) ? 2 * DZ1_CAP * L.H * 4 : 0);
    }
    // (sum, sumsq) pairs of a minibatch's advantages: adv_partial_kernel's blocks, and the stride between a prepared epoch's minibatches
    static int adv_stride(int64_t batch) { return (int)(ceil_div(batch, 1024) < ADV_BLOCKS ? ceil_div(batch, 1024) : ADV_BLOCKS); }

    PLayout L;
    int64_t o_offsets, o_epoch_part, o_wide_sq, o_dz1, o_fold, o_end;
    Workspace(void *ws, const PLayout &layout) : WorkspaceHeader(ws), L(layout) {
        o_offsets = BYTES + slab_bytes(L);
        o_epoch_part = o_offsets + OFFS_CAP * 4;
        o_wide_sq = o_epoch_part + EPOCH_PART_BYTES;
        o_dz1 = o_wide_sq + WIDE_SQ_SLOTS * 8;
        o_fold = (o_dz1 + dz1_cache_bytes(L) + 15) & ~(int64_t)15;
        o_end = o_fold + ((L.img_pi >= 0 || h256p_layout(L)) ? 3 * fold_stride() * 4 : 0);
    }
    int64_t bytes() const { return o_end; }  // tma_ppo_workspace_bytes

    float *defer_w2() const {  // OVERLAYS slabs DEFER_W2_SLAB and up; [net][h1 | dz2][W2_DEFER_ROWS][H]
        assert(defer_w2_fits(L));
        return slabs() + (int64_t)DEFER_W2_SLAB * L.P;
    }
    int32_t *offsets() const { return at<int32_t>(o_offsets); }       // [OFFS_CAP] buffer offset of every row of the prepared epoch(s)
    double *epoch_partials() const { return at<double>(o_epoch_part); }  // minibatch m of them: + 2 * m * adv_stride(batch_size)
    int n_sq_partials() const { return (int)ceil_div(L.P, 64); }
    double *sq_partials() const {  // where slab_reduce_kernel leaves its sum-of-squares partials (one per 64 parameters) for the optimizer step
        if (n_sq_partials() <= 256) return norm_partials();
        return n_sq_partials() <= WIDE_SQ_SLOTS ? at<double>(o_wide_sq) : nullptr;
    }
    template <class T> T *dz1_cache() const { return at<T>(o_dz1); }  // two-pass layouts: [net][DZ1_CAP][H] of bf16 or float
    // second half of the (parameters, exp_avg, exp_avg_sq) double buffer of AdamFold, and the snapshot a persistent launch's fallback restores:
    // 3 x fold_stride() floats, for the H = 64 fast-path layouts and h256p_layout only (no bytes otherwise)
    int64_t fold_stride() const { return ((int64_t)L.P + 3) & ~(int64_t)3; }
    float *fold_state() const { return at<float>(o_fold); }
};

}  // namespace tma
