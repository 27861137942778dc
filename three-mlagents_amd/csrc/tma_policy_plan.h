// tma_policy_plan.h -- WHICH kernel specialisation the policy's three dispatchers run for a shape, and with what launch geometry: plain structs
// and pure host functions (no HIP call, no global, no environment read), so that the selection is checkable without a GPU
// (tma_debug_plan_dispatch).  The launchers of tma_policy.hip (and tma_bf16.hip's, for plan_grad_bf) validate, call plan_*, record plan.id and
// launch what the plan says: every threshold and cap of the selection is written here, once.
// Included inside namespace tma by tma_policy.hip, after tma_ppo_types.h and tma_wide_bf16.h.
#pragma once

// Every environment switch the three dispatchers read (filled by read_switches in tma_policy.hip; tools/test_switches.sh runs each of them)
struct DispatchSwitches {
    bool force_wide;      // TMA_FORCE_WIDE, gradient: once per process.  Test hook: the column-parallel kernel at any batch size
    bool force_wide_now;  // TMA_FORCE_WIDE, tma_ppo_adam_step_local: on each call
    bool no_half;         // TMA_NO_HALF_GROUPS: once per process.  32-row groups throughout
    bool no_defer;        // TMA_NO_DEFER_W2: once per process.  The slab path throughout (small7 has no dW2 accumulators: it goes too)
    bool nw4;             // TMA_WIDE_NW4: on each call.  H = 256 single-pass shapes on four waves of 64 columns
    bool no_dz1;          // TMA_NO_DZ1_CACHE: on each call.  The two-pass kernels recompute the chain
    bool split3;          // tma_split3_eligible(L, count), which reads TMA_NO_SPLIT3: on each call
    int bf_debug;         // TMA_BF_DEBUG: once per process.  Phase mask of the bf16 wide kernel (HParams::debug)
    // the bf16 column-parallel gradient (plan_grad_bf), which also reads no_dz1
    bool bf_mt2;          // TMA_BF_MT2: once per process.  Development switch: 32-row groups throughout
    bool bf_nw4;          // TMA_BF_NW4: once per process.  A/B switch: every shape on four waves (the Ant width then takes the runtime-width kernel)
    int bf_npi;           // TMA_BF_NPI: once per process.  Development switch: policy-net block count (0: the measured split)
};

constexpr int LDS_LIMIT = 160 * 1024;         // dynamic LDS of one workgroup: what needs more is refused
constexpr int LDS_OPT_IN = 64 * 1024;         // ... and beyond this a kernel has to ask (hipFuncAttributeMaxDynamicSharedMemorySize)
constexpr int GENERIC_GRAD_LDS = 156 * 1024;  // the generic gradient kernel takes as many waves per block (up to 4) as fit this
constexpr int64_t WIDE_FWD_GROUP_CAP = 4096, GENERIC_FWD_BLOCK_CAP = 8192, H64_FWD_BLOCK_CAP = 2048;  // then grid-stride
constexpr int H64_HEAD_STAGE = 16 * 16;  // floats per wave (mode 4)
constexpr int64_t GENERIC_GRAD_BLOCK_CAP = MAX_GRAD_BLOCKS / 2;  // per net: one statistic slot per block

inline int fwd_smem_bytes(const PLayout &L, int wpb) {
    const int ldx = ((L.D + 3) & ~3) + 2, ld = L.H + 2;
    return wpb * (16 * (ldx + 2 * ld) + 32) * 4;
}
inline int grad_smem_bytes(const PLayout &L, int wpb) {
    const int ldx = ((L.D + 3) & ~3) + 2, ld = L.H + 2;
    return wpb * (16 * (ldx + 2 * ld + 34) + 16 * 8) * 4;
}
inline int fwd_wide_smem_bytes(const PLayout &L) {
    const int ldx = ((L.D + 3) & ~3) + 2, ld = L.H + 2;
    return 32 * (ldx + 2 * ld) * 4;
}
inline int grad_wide_smem_bytes(const PLayout &L, int nw = 4) {
    const int ldx = ((L.D + 3) & ~3) + 2, ld = L.H + 2;
    return (32 * (ldx + 2 * ld + 34 + 4) + 2 * 32 + 64 + nw * 2 * 2 * 256 + 2 * L.H + 32 + 2 * 32 + 32 * 32) * 4;  // (last terms: row_off_next, the Box heads' action tile)
}
inline bool wide_width(const PLayout &L) { return L.H == 128 || L.H == 192 || L.H == 256; }
// Only the generic one-wave-per-tile kernels (policy_fwd_kernel, ppo_grad_kernel) are templated on the activation: every tuned family below -- the
// H = 64 LDS-image kernels, the column-parallel ones, and what hangs on them (persistent epochs, the prologue optimizer fold, half groups, two
// passes, small7, the split) -- is tanh code, so each of their conditions asks this first
inline bool tanh_layout(const PLayout &L) { return L.act == ACT_TANH; }
// shapes the f32 column-parallel gradient kernel can take (from how many samples on it does: plan_grad, plan_opt)
inline bool grad_wide_f32_shape(const PLayout &L) { return tanh_layout(L) && !L.bf16 && wide_width(L) && grad_wide_smem_bytes(L) <= LDS_LIMIT; }
// the dW2 deferral buffer overlays the upper slabs of the workspace's slab area (Workspace::defer_w2): it must fit there
inline bool w2_defer_fits(const PLayout &L) { return Workspace::defer_w2_fits(L); }
// slab_reduce_kernel / wide_small_reduce_kernel leave one sum-of-squares partial per 64 parameters where the workspace has slots for them
inline bool sq_partials_fit(const PLayout &L) { return ceil_div(L.P, 64) <= WIDE_SQ_SLOTS; }

// ---- forward (mode 0: act, 1: values, 2: bootstrap, 3: evaluate_actions, 4: the head itself -- tma_policy_head; 0, 3 and 4 run both nets).
// It reads no switch.
enum class FwdFamily { Refused, H64, WideF32, WideBF16, Generic };
struct FwdPlan {
    FwdFamily family;
    bool cont;
    int ntw;  // column-parallel kernels: H / 64
    int64_t grid;
    int block, lds;  // (Refused: lds = what one wave's tile would need)
    int32_t id;      // TMA_DISPATCH_FWD_* [| TMA_DISPATCH_GRID_CAPPED]; NONE when refused
};
inline FwdPlan plan_fwd(const PLayout &L, int64_t n, int mode) {
    FwdPlan p{FwdFamily::Refused, L.cont != 0, L.H / 64, 0, 256, 0, TMA_DISPATCH_NONE};
    const int64_t tiles = ceil_div(n, 16), groups = ceil_div(n, 32);
    const int nets = (mode == 0 || mode == 3 || mode == 4) ? 2 : 1;
    if (tanh_layout(L) && L.img_pi >= 0) {  // both nets' weight images in LDS
        p.family = FwdFamily::H64, p.id = TMA_DISPATCH_FWD_H64;
        const int wpb = tiles >= 512 ? 4 : (tiles >= 64 ? 2 : 1);  // waves per block
        p.grid = ceil_div(tiles, wpb) < H64_FWD_BLOCK_CAP ? ceil_div(tiles, wpb) : H64_FWD_BLOCK_CAP;
        p.block = 64 * wpb, p.lds = nets * FWD_IMG * 4;
        if (mode == 4) p.lds += wpb * H64_HEAD_STAGE * 4;  // a wave's [16][A] head tile on its way to a coalesced store
    } else if (tanh_layout(L) && (L.bf16 || (wide_width(L) && fwd_wide_smem_bytes(L) <= LDS_LIMIT))) {  // column-parallel: row groups of 32, one block per group and net
        p.family = L.bf16 ? FwdFamily::WideBF16 : FwdFamily::WideF32;
        p.id = (L.bf16 ? (p.cont ? TMA_DISPATCH_FWD_BF16_NTW2_BOX : TMA_DISPATCH_FWD_BF16_NTW2_DISCRETE)
                       : (p.cont ? TMA_DISPATCH_FWD_F32_NTW2_BOX : TMA_DISPATCH_FWD_F32_NTW2_DISCRETE)) + (p.ntw - 2) |
               (groups > WIDE_FWD_GROUP_CAP ? TMA_DISPATCH_GRID_CAPPED : 0);
        p.grid = nets * (groups < WIDE_FWD_GROUP_CAP ? groups : WIDE_FWD_GROUP_CAP);
        p.lds = L.bf16 ? fwd_wide_bf_smem_bytes(L.D, L.H) : fwd_wide_smem_bytes(L);
    } else {  // one wave per 16-row tile: every width of a non-tanh layout, too
        int wpb = tiles >= 1024 ? 4 : 1;  // small batches: one wave per block so every CU gets work
        while (wpb > 1 && fwd_smem_bytes(L, wpb) > LDS_OPT_IN) wpb >>= 1;
        p.lds = fwd_smem_bytes(L, wpb);
        if (p.lds > LDS_LIMIT) return p;  // (check_dims accepts up to 4096 observations and 1024 hidden units: more than one wave's tile can hold)
        const int64_t blocks = ceil_div(tiles, wpb);
        p.family = FwdFamily::Generic;
        p.id = (wpb == 4 ? TMA_DISPATCH_FWD_GENERIC_W4 : (wpb == 2 ? TMA_DISPATCH_FWD_GENERIC_W2 : TMA_DISPATCH_FWD_GENERIC_W1)) |
               (blocks > GENERIC_FWD_BLOCK_CAP ? TMA_DISPATCH_GRID_CAPPED : 0);
        p.grid = blocks < GENERIC_FWD_BLOCK_CAP ? blocks : GENERIC_FWD_BLOCK_CAP;
        p.block = 64 * wpb;
    }
    return p;
}

// ---- minibatch gradient, bf16 column-parallel kernels (tma_bf16.hip launches what this returns).  It reads bf_mt2, bf_nw4, bf_npi and no_dz1.
constexpr int64_t BF_MT4_FROM = 4096;  // 64-row groups beyond this many samples
inline GradBfPlan plan_grad_bf(const PLayout &L, int64_t count, const DispatchSwitches &sw) {
    GradBfPlan p{};
    // observation width classes: <= 16, <= 32: dW1 in registers (one / two k-tiles); 33..64, 161..192 (Crawler's 172) and 97..128 with a Box head at
    // H = 256 (the reference's ant task): two passes with 2 / 6 / 4 layer-1 k-steps; any other width: runtime width, dW1 in place in the slab
    const int variant = L.D <= 16 ? 0 : (L.D <= 32 ? 1 : (L.D <= 64 ? 2 : ((L.D > 160 && L.D <= 192) ? 3 : ((L.D > 96 && L.D <= 128 && L.cont && L.H == 256) ? 5 : 4))));
    // observations of up to 32 floats: 64-row groups (half the weight bytes, barriers and latency chains per sample); wider ones keep
    // 32-row groups (their observation images would not fit next to 64-row activation images).  Minibatches too small to give every block a
    // 64-row group take 32-row groups as well: twice the workgroups on a launch that is all latency
    p.mt = (variant <= 1 && !sw.bf_mt2 && L.H != 192 && count > BF_MT4_FROM) ? 4 : 2;  // (H = 192: three column tiles per wave do not split in halves)
    const int smemw = grad_wide_bf_smem_bytes(L.D, L.H, p.mt);
    const int64_t groups = ceil_div(count, 16 * p.mt);
    // eight waves (two per SIMD, 32 columns each): 64-row groups of the Discrete layouts with observations of up to 16 floats at H = 256
    // (GridWorld, Push, Ball3D, WallJump), and the two-pass Box layouts of the Ant and Crawler widths at H = 256
    const bool eight_kt1 = !sw.bf_nw4 && p.mt == 4 && variant == 0 && !L.cont && L.H == 256;
    const bool eight_ks = !sw.bf_nw4 && (variant == 5 || (variant == 3 && L.cont && L.H == 256));
    // 256 blocks = one per CU.  A policy-net row group costs 1.15-1.3x a value-net one (the loss), so the policy net gets 136 to 144 of the
    // blocks (the Categorical loss is cheaper than the DiagGaussian one; the eight-wave kernel shares a tile's loss between two waves: swept
    // 124 .. 160, best 136 .. 140); with fewer row groups than that, one block per group
    const int cap_pi = sw.bf_npi > 0 ? sw.bf_npi : (L.cont ? 144 : (eight_kt1 ? 140 : 136)), cap_vf = 256 - cap_pi;
    p.n_pi = (int)(groups < cap_pi ? groups : cap_pi), p.n_vf = (int)(groups < cap_vf ? groups : cap_vf);
    p.waves = (eight_kt1 || eight_ks) ? 8 : 4, p.block = 64 * p.waves;
    // two-pass layouts: minibatches that fit the dz1 cache take PASS 0 (which leaves dz1 there) + PASS 2 (dW1 from the cache) instead of
    // PASS 0 + PASS 1 (dW1 from a recomputed forward / backward chain); the results are bit-identical
    const bool cached = bf_two_pass(L) && count <= DZ1_CAP && !sw.no_dz1;
    if (variant == 4 || (variant == 5 && sw.bf_nw4)) {
        p.id = TMA_DISPATCH_GRAD_BF16_RUNTIME, p.pass = BfPass::Single, p.zero_w1 = true, p.lds = smemw;
    } else if (variant <= 1) {
        p.kt1c = variant + 1, p.ks1c = 1, p.pass = BfPass::Single;
        p.id = eight_kt1 ? TMA_DISPATCH_GRAD_BF16_KT1_MT4_W8
                         : (variant == 0 ? (p.mt == 4 ? TMA_DISPATCH_GRAD_BF16_KT1_MT4 : TMA_DISPATCH_GRAD_BF16_KT1_MT2)
                                         : (p.mt == 4 ? TMA_DISPATCH_GRAD_BF16_KT2_MT4 : TMA_DISPATCH_GRAD_BF16_KT2_MT2));
        p.lds = eight_kt1 ? smemw + (L.H / 32) * 1024 + 12 * 4 * 5 * 8 : smemw;  // + the head fragments + the statistics slots of the row-lane loss (64 in all)
    } else {
        p.ks1c = variant == 2 ? 2 : (variant == 3 ? 6 : 4), p.pass = cached ? BfPass::Cached : BfPass::Recompute;
        p.id = variant == 2 ? (cached ? TMA_DISPATCH_GRAD_BF16_KS2_CACHED : TMA_DISPATCH_GRAD_BF16_KS2_RECOMPUTE)
             : variant == 5 ? (cached ? TMA_DISPATCH_GRAD_BF16_KS4_W8_CACHED : TMA_DISPATCH_GRAD_BF16_KS4_W8_RECOMPUTE)
             : eight_ks     ? (cached ? TMA_DISPATCH_GRAD_BF16_KS6_W8_CACHED : TMA_DISPATCH_GRAD_BF16_KS6_W8_RECOMPUTE)
                            : (cached ? TMA_DISPATCH_GRAD_BF16_KS6_CACHED : TMA_DISPATCH_GRAD_BF16_KS6_RECOMPUTE);
        p.lds = eight_ks ? smemw + 4 * 4 * 5 * 8 : smemw;  // + the statistics of four more waves
    }
    return p;
}

// ---- minibatch gradient
enum class GradFamily { Refused, H64Small, H64, BF16, BF16X3, WideF32, Generic };
enum class GradReduce { None, Slab, WideSmall };
struct GradPlan {
    GradFamily family;
    bool cont;
    bool normalize;  // normalize_advantage, and more than one sample
    // pre-launches: adv_partial_kernel (sample offsets into the workspace cache when offs_cache, + partials when normalize), adv_final_kernel
    bool offs_cache, adv_partial, adv_final;
    // WideF32.  kt1: k-tiles of dW1 in registers -- 1 / 2: D <= 16 / 32; 7: small7; 11 (Crawler's 172 observations) and 107 (Ant-v5's 105: "7 in
    // two passes"): a second pass that keeps only dW1; 0: any other width accumulates dW1 in place in the slab, behind slab_zero_w1_kernel
    int kt1, ntw;
    bool half;        // 16-row half groups: the reference's literal batch_size = 256 on 32 workgroups instead of 16
    bool eight;       // H = 256, single-pass shapes: eight waves of 32 columns
    bool defer_w2;    // dW2 left to wide_small_reduce_kernel through the deferral buffer (half groups on eight waves: <= 64 slabs in use)
    bool dz1_cached;  // two passes: the second takes dz1 from the workspace cache instead of recomputing the chain
    int n_pi, n_vf;   // blocks = slabs of the policy net; the value net's blocks use the first n_vf of them
    int64_t groups;
    // WideF32, BF16 (the first dominant launch) and Generic: the launch.  lds = -1: the family's own launcher picks the dominant kernel's geometry
    // (tma_h64.hip, tma_split3.hip) and grid / block are the slab reduction's that follows.  Refused: lds = one wave's tile
    int64_t grid;
    int block, lds;
    GradBfPlan bf;  // BF16: what tma_launch_grad_wide_bf launches
    GradReduce reduce;
    int32_t id;  // TMA_DISPATCH_GRAD_* [| TMA_DISPATCH_GRID_CAPPED]; NONE when refused
};
inline GradPlan plan_grad(const PLayout &L, bool cont, int64_t count, bool prepared, bool normalize_advantage, const DispatchSwitches &sw) {
    GradPlan p{};
    p.cont = cont, p.normalize = normalize_advantage && count > 1, p.ntw = L.H / 64;
    const int64_t tiles = ceil_div(count, 16);
    const bool h64 = tanh_layout(L) && L.img_pi >= 0 && tiles >= 16;  // >= 256 samples: persistent LDS-image kernel; smaller batches: generic kernel
    const bool wide_f32 = grad_wide_f32_shape(L) && (tiles >= 8 || sw.force_wide);
    // offsets cache: written by the advantage pass, read by every gradient kernel (saves the permutation arithmetic per sample);
    // a prepared epoch (tma_ppo_epoch_prepare) left offsets and partials in the workspace
    p.offs_cache = !prepared && count <= OFFS_CAP && (p.normalize || L.bf16);
    p.adv_partial = !prepared && (p.normalize || p.offs_cache);
    p.adv_final = p.normalize && !h64 && !L.bf16 && !wide_f32;  // the H = 64 and the column-parallel kernels fold the partials themselves
    p.grid = ceil_div(L.P, 64), p.block = 256, p.lds = -1, p.reduce = GradReduce::Slab;
    if (h64) {  // register-accumulating persistent kernel (tma_h64.hip: one tile per wave up to 2048 samples)
        p.family = tiles <= H64_BLOCKS ? GradFamily::H64Small : GradFamily::H64;
        p.id = tiles <= H64_BLOCKS ? TMA_DISPATCH_GRAD_H64_SMALL : TMA_DISPATCH_GRAD_H64;
    } else if (L.bf16) {  // column-parallel bf16-MFMA kernel (tma_bf16.hip)
        p.family = GradFamily::BF16, p.bf = plan_grad_bf(L, count, sw);
        p.id = p.bf.id, p.n_pi = p.bf.n_pi, p.n_vf = p.bf.n_vf;
        p.grid = p.n_pi + p.n_vf, p.block = p.bf.block, p.lds = p.bf.lds;  // (of every launch of the leaf)
    } else if (wide_f32 && sw.split3) {  // mfma_dtype = 2: the same update on the bf16 MFMA, every operand as three bf16 terms
        p.family = GradFamily::BF16X3, p.id = TMA_DISPATCH_GRAD_BF16X3;
    } else if (wide_f32) {  // column-parallel register-accumulating kernel
        p.family = GradFamily::WideF32;
        const bool small7 = L.H == 256 && L.D > 32 && L.D <= 112 && count <= 1024 && !sw.no_half && !sw.nw4 && !sw.no_defer && w2_defer_fits(L);
        // (at 2048 samples the doubled slab count costs more than the shorter groups save: 79.6 against 76.6 us per call)
        p.half = (L.D <= 32 || small7) && count <= 1024 && !sw.no_half;
        p.groups = ceil_div(count, p.half ? 16 : 32);  // one row group per block while there are CUs to spare, then grid-stride
        const int cap_pi = cont ? 136 : 128, cap_vf = 256 - cap_pi;  // measured: the Categorical head leaves the two nets balanced
        p.n_pi = (int)(p.groups < cap_pi ? p.groups : cap_pi), p.n_vf = (int)(p.groups < cap_vf ? p.groups : cap_vf);
        p.kt1 = L.D <= 16 ? 1 : (L.D <= 32 ? 2 : (small7 ? 7 : ((L.D > 160 && L.D <= 176) ? 11 : ((f32_two_pass(L) && L.D <= 112) ? 107 : 0))));
        p.eight = L.H == 256 && (p.kt1 == 1 || p.kt1 == 2 || p.kt1 == 7) && !sw.nw4;
        p.defer_w2 = p.half && p.eight && !sw.no_defer && p.n_pi <= 64 && p.groups * 16 <= W2_DEFER_ROWS && w2_defer_fits(L);
        // (as on the bf16 path) minibatches that fit the dz1 cache: chain pass + dW1 from the cached operands; else chain + recompute
        p.dz1_cached = f32_two_pass(L) && (p.kt1 == 11 || p.kt1 == 107) && count <= DZ1_CAP && !sw.no_dz1;
        p.grid = p.n_pi + p.n_vf, p.block = p.eight ? 512 : 256, p.lds = grad_wide_smem_bytes(L, p.eight ? 8 : 4);
        if (p.defer_w2) p.reduce = GradReduce::WideSmall;
        const bool k2 = p.kt1 == 2;
        if (p.kt1 == 7) p.id = TMA_DISPATCH_GRAD_F32_SMALL7;
        else if (p.kt1 == 11) p.id = p.dz1_cached ? TMA_DISPATCH_GRAD_F32_KT11_CACHED : TMA_DISPATCH_GRAD_F32_KT11_RECOMPUTE;
        else if (p.kt1 == 107) p.id = p.dz1_cached ? TMA_DISPATCH_GRAD_F32_KT107_CACHED : TMA_DISPATCH_GRAD_F32_KT107_RECOMPUTE;
        else if (p.kt1 == 0) p.id = TMA_DISPATCH_GRAD_F32_KT0;
        else if (!p.eight) p.id = p.half ? (k2 ? TMA_DISPATCH_GRAD_F32_KT2_HALF_W4 : TMA_DISPATCH_GRAD_F32_KT1_HALF_W4)
                                         : (k2 ? TMA_DISPATCH_GRAD_F32_KT2_FULL_W4 : TMA_DISPATCH_GRAD_F32_KT1_FULL_W4);
        else if (!p.half) p.id = k2 ? TMA_DISPATCH_GRAD_F32_KT2_FULL_W8 : TMA_DISPATCH_GRAD_F32_KT1_FULL_W8;
        else if (p.defer_w2) p.id = k2 ? TMA_DISPATCH_GRAD_F32_KT2_HALF_W8_DEFER : TMA_DISPATCH_GRAD_F32_KT1_HALF_W8_DEFER;
        else p.id = k2 ? TMA_DISPATCH_GRAD_F32_KT2_HALF_W8_SLAB : TMA_DISPATCH_GRAD_F32_KT1_HALF_W8_SLAB;
    } else {  // one wave per 16-row tile, float atomics into the gradient: no reduction
        p.reduce = GradReduce::None;
        int wpb = tiles >= 512 ? 4 : 1;  // waves per block
        while (wpb > 1 && grad_smem_bytes(L, wpb) > GENERIC_GRAD_LDS) wpb--;
        p.lds = grad_smem_bytes(L, wpb);
        if (p.lds > LDS_LIMIT) return p;  // Refused
        const int64_t blocks = ceil_div(tiles, wpb);  // per net
        p.family = GradFamily::Generic;
        p.id = (wpb == 4 ? TMA_DISPATCH_GRAD_GENERIC_W4 : (wpb == 3 ? TMA_DISPATCH_GRAD_GENERIC_W3 : (wpb == 2 ? TMA_DISPATCH_GRAD_GENERIC_W2 : TMA_DISPATCH_GRAD_GENERIC_W1))) |
               (blocks > GENERIC_GRAD_BLOCK_CAP ? TMA_DISPATCH_GRID_CAPPED : 0);
        p.grid = 2 * (blocks < GENERIC_GRAD_BLOCK_CAP ? blocks : GENERIC_GRAD_BLOCK_CAP), p.block = 64 * wpb;
    }
    return p;
}

// ---- optimizer step: tma_ppo_adam_step (local = false) and tma_ppo_adam_step_local, which takes the gradient's sum-of-squares partials from the
// reduction of the last tma_ppo_minibatch_grad (last_count samples) where that ended in one, and is tma_ppo_adam_step otherwise
enum class OptKernels { ScatterH64, ScatterWide, Small, Adam };
struct OptPlan {
    OptKernels kernels;
    bool falls_through;  // a _local call that runs the global step
    int64_t grid;        // of the kernel that steps the parameters
    int block;
    int32_t id;  // TMA_DISPATCH_OPT_*
};
inline OptPlan plan_opt(const PLayout &L, bool local, int64_t last_count, const DispatchSwitches &sw) {
    const bool sq = sq_partials_fit(L);
    // "did the gradient end in a slab reduction", as this entry point has always asked it: from 256 samples (H = 64) and 128 samples (f32
    // column-parallel) on.  plan_grad reduces from 241 (16 tiles) and 113 (8 tiles) on; in between the global step runs, which is right for any gradient.
    const bool red_h64 = tanh_layout(L) && L.img_pi >= 0 && last_count >= 256;  // (a non-tanh layout: the generic gradient kernel at every count, no reduction)
    const bool red_wide = L.bf16 || (grad_wide_f32_shape(L) && last_count >= 128 && !sw.force_wide_now);
    OptPlan p{OptKernels::Adam, false, ceil_div(L.P, 256), 256, TMA_DISPATCH_OPT_ADAM};
    if (local && (red_h64 || red_wide) && sq && last_count >= 1) {
        p.kernels = red_h64 ? OptKernels::ScatterH64 : OptKernels::ScatterWide;
        p.id = red_h64 ? TMA_DISPATCH_OPT_LOCAL_SCATTER_H64 : TMA_DISPATCH_OPT_LOCAL_SCATTER_WIDE;
        return p;
    }
    p.falls_through = local;
    const bool scat_h64 = L.img_pi >= 0 && L.P <= 64 * 256, scat_wide = L.bf16 || L.fr_pi >= 0;
    if (sq && (scat_h64 || scat_wide)) {  // layouts whose derived copies the optimizer kernel scatters itself
        p.kernels = scat_h64 ? OptKernels::ScatterH64 : OptKernels::ScatterWide;
        p.id = scat_h64 ? TMA_DISPATCH_OPT_SCATTER_H64 : TMA_DISPATCH_OPT_SCATTER_WIDE;
    } else if (L.P <= 32768) {  // one workgroup
        p.kernels = OptKernels::Small, p.grid = 1, p.block = 1024, p.id = TMA_DISPATCH_OPT_SMALL;
    } else {
        p.grid = ceil_div(L.P, 1024) < 256 ? ceil_div(L.P, 1024) : 256;
    }
    return p;
}
