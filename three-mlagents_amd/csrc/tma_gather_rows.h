// tma_gather_rows.h -- the row walk shared by the gather kernels (tma_gather.hip: tma_rollout_gather; tma_replay.hip: tma_replay_sample):
// a wave copies a block of scattered source rows into its contiguous span of the output, stores coalesced.
#pragma once
#include "tma_common.h"

namespace tma {

constexpr int GATHER_WAVES = 4;  // waves per workgroup, each on a row block of its own

// rows [0, rows) of a wave's block, W = width / VEC vectors each: dst is the block's contiguous [rows][W] span, src the plane's base; `off` is
// lane l's plane row (valid in lanes < rows).  Four vectors a lane are loaded before the first is stored.  (Measured and dropped: eight loads in
// flight, and the scalars' stores moved behind the walk so that their loads and the walk's share one round trip -- 17.6 / 23.6 us against
// 16.8 / 22.6 at the two large shapes of DESIGN.md section 15: the round trips of one block are not what bounds the kernel.)
template <class V>
__device__ __forceinline__ void gather_rows(const V *__restrict__ src, V *__restrict__ dst, int off, int rows, int W, int lane) {
    const int n = rows * W;
    const float inv_w = 1.0f / (float)W;  // e / W without an integer division: e < 64 * 4096 is exact in f32, the quotient is off by one at the most
    for (int e0 = 0; e0 < n; e0 += 4 * 64) {
        V v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = e0 + 64 * q + lane;
            const int ec = e < n ? e : 0;  // (every lane takes part in the cross-lane read; lanes behind the span read element 0 and store nothing)
            int row = (int)((float)ec * inv_w), c = ec - row * W;
            if (c < 0) row--, c += W;
            if (c >= W) row++, c -= W;
            const int o = __shfl(off, row, 64);
            v[q] = src[(int64_t)o * W + c];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = e0 + 64 * q + lane;
            if (e < n) dst[e] = v[q];
        }
    }
}

}  // namespace tma
