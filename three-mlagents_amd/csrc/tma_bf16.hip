// tma_bf16.hip -- PPO minibatch gradient for 128 / 192 / 256-wide policies on the bf16 MFMA (tma_policy_dims.mfma_dtype = 1;
// BASELINE.json configs[2] "PPO MLP(256,256) bf16").  The kernel body lives in tma_wide_bf16.h (shared with the forward kernels of
// tma_policy.hip); this translation unit instantiates the gradient kernel and picks the variant for a policy shape.
//
// Replaces, for the reference's default net_arch (/root/reference/backend/mlagents/training.py:363-365), what SB3's PPO.train computes
// per minibatch between RolloutBuffer.get and optimizer.step (third party).
#include "tma_ppo_types.h"

#include <cstdlib>
#include <type_traits>

namespace tma {
#ifdef TMA_BF_PHASE_TICKS
__device__ unsigned long long g_bf_ticks[2][16];
#endif
#include "tma_wide_bf16.h"
}  // namespace tma

#ifdef TMA_BF_PHASE_TICKS
// diagnostic build only: read (reset != 0: clear) the per-phase cycle sums of the bf16 gradient kernel
extern "C" int tma_debug_bf_ticks(unsigned long long *out32, int reset) {
    if (reset) {
        unsigned long long z[32] = {0};
        return hipMemcpyToSymbol(HIP_SYMBOL(tma::g_bf_ticks), z, sizeof(z)) == hipSuccess ? 0 : 1;
    }
    return hipMemcpyFromSymbol(out32, HIP_SYMBOL(tma::g_bf_ticks), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : 1;
}
#endif

using namespace tma;

// The runtime-to-template mapping of a plan (plan_grad_bf, tma_policy_plan.h): every leaf is one kernel form (single pass) or one triple
// (PASS 0, then PASS 2 from the dz1 cache or PASS 1 on a recomputed chain).  The eight-wave forms exist for one head and H = 256 only.
template <bool C, int NTW, typename Launch>
static int launch_bf_leaf(const GradBfPlan &p, bf16_t *dz1, Launch launch) {
    constexpr int MT4 = NTW % 2 == 0 ? 4 : 2;  // (H = 192 is never planned with 64-row groups)
    auto two = [&](auto k0, auto k2, auto k1) -> int {
        const int rc = launch(k0, dz1);
        if (rc) return rc;
        return dz1 ? launch(k2, dz1) : launch(k1, nullptr);
    };
    switch (p.id) {
    case TMA_DISPATCH_GRAD_BF16_KT1_MT2: return launch(ppo_grad_wide_bf_kernel<C, NTW, 2, 1, 1, 0>, nullptr);
    case TMA_DISPATCH_GRAD_BF16_KT1_MT4: return launch(ppo_grad_wide_bf_kernel<C, NTW, MT4, 1, 1, 0>, nullptr);
    case TMA_DISPATCH_GRAD_BF16_KT2_MT2: return launch(ppo_grad_wide_bf_kernel<C, NTW, 2, 2, 1, 0>, nullptr);
    case TMA_DISPATCH_GRAD_BF16_KT2_MT4: return launch(ppo_grad_wide_bf_kernel<C, NTW, MT4, 2, 1, 0>, nullptr);
    case TMA_DISPATCH_GRAD_BF16_KS2_CACHED:
    case TMA_DISPATCH_GRAD_BF16_KS2_RECOMPUTE:
        return two(ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 2, 0>, ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 2, 2>, ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 2, 1>);
    case TMA_DISPATCH_GRAD_BF16_KS6_CACHED:
    case TMA_DISPATCH_GRAD_BF16_KS6_RECOMPUTE:
        return two(ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 6, 0>, ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 6, 2>, ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 6, 1>);
    case TMA_DISPATCH_GRAD_BF16_RUNTIME: return launch(ppo_grad_wide_bf_kernel<C, NTW, 2, 0, 0, 0>, nullptr);
    default: break;
    }
    if constexpr (!C && NTW == 4) {  // GridWorld, Push, Ball3D, WallJump (measured round 4, one box: 285 -> 246-255 us per 131 072 samples)
        if (p.id == TMA_DISPATCH_GRAD_BF16_KT1_MT4_W8) return launch(ppo_grad_wide_bf_kernel<false, 2, 4, 1, 1, 0, 8>, nullptr);
    }
    if constexpr (C && NTW == 4) {  // the Crawler width (six layer-1 k-steps) and the Ant width (four)
        if (p.id == TMA_DISPATCH_GRAD_BF16_KS6_W8_CACHED || p.id == TMA_DISPATCH_GRAD_BF16_KS6_W8_RECOMPUTE)
            return two(ppo_grad_wide_bf_kernel<true, 2, 2, 0, 6, 0, 8>, ppo_grad_wide_bf_kernel<true, 2, 2, 0, 6, 2, 8>, ppo_grad_wide_bf_kernel<true, 2, 2, 0, 6, 1, 8>);
        if (p.id == TMA_DISPATCH_GRAD_BF16_KS4_W8_CACHED || p.id == TMA_DISPATCH_GRAD_BF16_KS4_W8_RECOMPUTE)
            return two(ppo_grad_wide_bf_kernel<true, 2, 2, 0, 4, 0, 8>, ppo_grad_wide_bf_kernel<true, 2, 2, 0, 4, 2, 8>, ppo_grad_wide_bf_kernel<true, 2, 2, 0, 4, 1, 8>);
    }
    return fail(TMA_ERR_INVALID, "internal: bf16 gradient plan %d has no kernel for this head and width", (int)p.id);
}

int tma_launch_grad_wide_bf(const float *params, const Rollout &R, const Minibatch &M, const HParams &hpar, const Workspace &ws, const GradBfPlan &p,
                            hipStream_t s) {
    const PLayout &L = ws.L;
    float *const slabs = ws.slabs();
    if (p.zero_w1) {  // runtime observation width: dW1 accumulates in place in the slab
        const int zrc = tma_launch_slab_zero_w1(slabs, p.n_pi, L, s);
        if (zrc) return zrc;
    }
    bf16_t *const dz1 = p.pass == BfPass::Cached ? ws.dz1_cache<bf16_t>() : nullptr;  // two-pass layouts
    auto launch = [&](auto k, bf16_t *dz) -> int {
        TMA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds));
        k<<<dim3((unsigned)(p.n_pi + p.n_vf)), dim3((unsigned)p.block), p.lds, s>>>(params, L, R, M, hpar, ws.adv(), slabs, ws.stats(), p.n_pi, dz, DZ1_CAP * L.H);
        return TMA_OK;
    };
    auto with_ntw = [&](auto cont) -> int {
        constexpr bool C = decltype(cont)::value;
#ifdef TMA_BF_DEV  // development builds: discrete heads at H = 256 only (a third of the instantiations)
        return launch_bf_leaf<C, 4>(p, dz1, launch);
#else
        return L.H == 256 ? launch_bf_leaf<C, 4>(p, dz1, launch) : (L.H == 192 ? launch_bf_leaf<C, 3>(p, dz1, launch) : launch_bf_leaf<C, 2>(p, dz1, launch));
#endif
    };
#ifdef TMA_BF_DEV
    const int lrc = with_ntw(std::false_type{});
#else
    const int lrc = L.cont ? with_ntw(std::true_type{}) : with_ntw(std::false_type{});
#endif
    if (lrc) return lrc;
    TMA_LAUNCH_CHECK();
    return TMA_OK;
}
