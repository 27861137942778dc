// tma_rollout_plan.h -- WHICH kernel family tma_rollout_collect / tma_rollout_collect_norm run for a shape, and with what launch geometry: plain
// structs and pure host functions (no HIP call, no global, no environment read), so that the selection is checkable without a GPU
// (tma_debug_plan_rollout).  The entry points of tma_rollout.hip validate, call plan_rollout, record the plan and run it: every threshold of the
// selection is written here, once.
// Included inside namespace tma by tma_rollout.hip, after the chunk kernels and the LDS totals their launchers pass.
#pragma once

// Every environment switch of the rollout driver (filled once per process by read_rollout_switches in tma_rollout.hip; tools/test_switches.sh runs them)
struct RolloutSwitches {
    bool no_wide_fused;  // TMA_NO_WIDE_FUSED: test hook.  Every 256-wide shape on the per-step composition
    bool no_cont_f32;    // TMA_NO_CONT_F32_FUSED: A/B switch.  The f32 Box shapes on the per-step composition
    bool cont_two_net;   // TMA_CONT_TWO_NET: A/B switch.  The bf16 Box shapes on the chunk with both nets in the step loop (Bf16BoxTwoNet)
    bool cont_serial;    // TMA_CONT_SERIAL: the Box families' value / bootstrap launches on the caller's stream (no overlap)
    int wide_f32_rows;   // TMA_WIDE_F32_ROWS: 8 / 16 force F32Disc's tile rows (16: BrickBreak and the normalised form go per-step)
    int wide_rows;       // TMA_WIDE_ROWS: 16 / 32 force Bf16Disc's rows per block
    int cont_rows;       // TMA_CONT_ROWS: 16 / 32 force Bf16BoxPi's rows per block
    bool roll2;          // TMA_ROLL2: A/B switch.  H64 on the two-wave kernel
    bool roll4;          // TMA_ROLL4: A/B switch.  H64 on the four-wave kernel
    bool no_norm_fused;  // TMA_NO_NORM_FUSED: A/B switch and test hook.  No VecNormalize step inside a chunk kernel
};

constexpr int LDS_LIMIT = 160 * 1024, LDS_OPT_IN = 64 * 1024;  // (as in tma_policy_plan.h) dynamic LDS of a workgroup; beyond the second a kernel has to ask
constexpr int64_t WIDE_BF16_ROWS16_MAX = 4096;  // bf16 families: 16 envs per block while 32 would leave CUs idle (<= 256 blocks of 16), else 32
constexpr int64_t WIDE_F32_ROWS8_MAX = 2048;    // F32Disc: tiles of 8 envs while every env gets its own block round, else 16; BrickBreak runs on 8 only
constexpr int64_t BOX_F32_MAX = 4096;           // F32Box: two block rounds of 8-env tiles; beyond that the per-step composition
constexpr int64_t H64_ONE_WAVE_TILES = 1024;    // H64: from this many 16-env tiles on, four tiles a workgroup on one wave each; below, one tile per workgroup
// the VecNormalize step inside the chunk: while the statistics move the vector is ONE tile (the moments of a step are one workgroup's work);
// frozen statistics: rows are independent, any number of tiles up to the kernel's own cap
constexpr int64_t NORM_FUSED_TRAIN_MAX = 8, NORM_FUSED_DISC_MAX = WIDE_F32_ROWS8_MAX, NORM_FUSED_CONT_MAX = BOX_F32_MAX;

// which tasks a family's kernels are instantiated for: the plan's eligibility and the launchers' `if constexpr` guards
template <class T>
constexpr bool h64_task = T::FUSED_ROLLOUT && T::USES_MT && T::NACT > 0;  // GridWorld, Push, Ball3D, WallJump, Bicycle, Glider
template <class T>
constexpr bool wide_disc_task = T::FUSED_ROLLOUT && T::OBS <= 32 && T::NACT > 0;
template <class T>
constexpr bool wide_f32_task = wide_disc_task<T> || T::ID == TMA_TASK_BRICKBREAK;  // (BrickBreak's 45 observations: on the 8-env tiles only)
template <class T>
constexpr bool wide_box_task = T::FUSED_ROLLOUT && T::NACT == 0 && T::ADIM <= 32 && !T::USES_MT && T::OBS <= 192;  // the Crawler / Ant shapes
template <class T>
constexpr bool two_net_task = T::FUSED_ROLLOUT && T::NACT == 0 && T::ADIM <= 32 && !T::USES_MT && ((T::OBS + 31) / 32) % 2 == 0;
// a task whose env step needs more registers than a wave of an eight-wave workgroup has (256) stays on the four-wave kernel: T::ROLL8 = false
template <class T, class = void>
struct roll8_task : std::true_type {};
template <class T>
struct roll8_task<T, std::enable_if_t<!T::ROLL8>> : std::false_type {};

enum class RolloutFamily { PerStep = 0, H64 = 1, Bf16Disc = 2, Bf16BoxTwoNet = 3, Bf16BoxPi = 4, F32Disc = 5, F32Box = 6 };  // TMA_ROLLOUT_FAMILY_*
enum class RolloutNorm { None = 0, Training = 1, Frozen = 2 };                                                               // TMA_ROLLOUT_PLAN_NORM_*
struct RolloutPlan {
    RolloutFamily family = RolloutFamily::PerStep;
    int waves = 0;               // H64: waves per 16-env tile -- 8, 4, 2, or 1 (four tiles a workgroup)
    int rows = 0;                // envs per tile or group: 8, 16 or 32 (PerStep: 0)
    bool batched_value = false;  // policy-only chunk: ONE value and ONE bootstrap launch per chunk, chunks capped at the terminal-observation slots
    bool overlap = false;        // Box families: those two launches on a side stream, the slots used as two halves in turn
    bool norm_in_chunk = false;  // the VecNormalize step runs inside the chunk kernel
    int64_t grid = 1;            // of the chunk kernel (PerStep launches no chunk: 1, 64, 0 -- its launches are tma_policy_plan.h's)
    int block = 64, lds = 0;
};

template <class T>
inline RolloutPlan plan_rollout_task(const PLayout &L, const tma_policy_dims &d, int64_t N, bool is_reset, int terminal_obs_slots, RolloutNorm norm,
                                     const RolloutSwitches &sw) {
    using F = RolloutFamily;
    // every fused chunk kernel is tanh code, starts from a reset env handle and takes the task's own observation and action widths
    const bool shape = L.act == ACT_TANH && is_reset && d.obs_dim == T::OBS;
    const bool acts = T::NACT > 0 && d.act_dim == T::NACT;
    const bool disc = wide_disc_task<T> && !d.continuous && acts, box = wide_box_task<T> && d.continuous && d.act_dim == T::ADIM;
    const bool brick = T::ID == TMA_TASK_BRICKBREAK && !d.continuous && acts && N <= WIDE_F32_ROWS8_MAX && sw.wide_f32_rows != 16;
    const bool wide = shape && !sw.no_wide_fused && L.H == 256, wide_bf16 = wide && L.bf16 && (disc || box), wide_f32 = wide && !L.bf16 && L.img_pi < 0;
    RolloutPlan p;
    // the precedence: Box pi-only bf16 or Box f32; bf16 wide (Discrete, or the two-net Box chunk under its switch); f32 wide Discrete; H64; per-step
    if (wide_bf16 && box && !sw.cont_two_net) p.family = F::Bf16BoxPi;
    else if (wide_f32 && box && !sw.no_cont_f32 && N <= BOX_F32_MAX) p.family = F::F32Box;
    else if (wide_bf16) p.family = box ? F::Bf16BoxTwoNet : F::Bf16Disc;
    else if (wide_f32 && (disc || brick)) p.family = F::F32Disc;
    else if (shape && L.img_pi >= 0 && h64_task<T> && acts) p.family = F::H64;
    if (norm != RolloutNorm::None) {  // under VecNormalize: the two f32 policy-only families with the step inside the chunk, or the per-step composition
        const int64_t cap = norm == RolloutNorm::Training ? NORM_FUSED_TRAIN_MAX : (p.family == F::F32Disc ? NORM_FUSED_DISC_MAX : NORM_FUSED_CONT_MAX);
        p.norm_in_chunk = !sw.no_norm_fused && N <= cap && (p.family == F::F32Box || (p.family == F::F32Disc && sw.wide_f32_rows != 16));
        if (!p.norm_in_chunk) p.family = F::PerStep;
    }
    const int norm_lds = p.norm_in_chunk ? vn_chunk_lds_doubles(T::OBS) * 8 : 0;  // its float64 statistics and scratch behind the float images
    const bool rows16 = N <= WIDE_BF16_ROWS16_MAX;
    p.block = 512;
    switch (p.family) {
    case F::PerStep: return RolloutPlan{};
    case F::H64: {
        const int64_t tiles = ceil_div(N, 16);
        p.waves = tiles >= H64_ONE_WAVE_TILES ? 1 : (sw.roll2 ? 2 : ((sw.roll4 || !roll8_task<T>::value) ? 4 : 8));
        p.rows = 16, p.grid = p.waves == 1 ? ceil_div(tiles, 4) : tiles, p.block = p.waves == 1 ? 256 : 64 * p.waves, p.lds = h64_chunk_lds_bytes(p.waves);
        return p;
    }
    case F::Bf16Disc:
        p.rows = (sw.wide_rows ? sw.wide_rows == 16 : rows16) ? 16 : 32, p.lds = p.rows == 16 ? WideLds<16>::bytes() : WideLds<32>::bytes();
        break;
    case F::Bf16BoxTwoNet:
        p.rows = 32;
        if constexpr (two_net_task<T>) p.lds = WideContLds<T>::bytes();
        break;
    case F::Bf16BoxPi:
        p.rows = (sw.cont_rows ? sw.cont_rows == 16 : rows16) ? 16 : 32, p.batched_value = true;
        if constexpr (wide_box_task<T>) p.lds = p.rows == 16 ? WideContPiLds<T, 16>::bytes() : WideContPiLds<T, 32>::bytes();
        break;
    case F::F32Disc:
        p.rows = (sw.wide_f32_rows ? sw.wide_f32_rows == 8 : N <= WIDE_F32_ROWS8_MAX) ? 8 : 16, p.batched_value = true;
        p.block = 256, p.lds = wide_f32_lds_bytes<T>(p.rows) + norm_lds;
        break;
    case F::F32Box:
        p.rows = 8, p.batched_value = true, p.block = 256;
        if constexpr (wide_box_task<T>) p.lds = WideContF32Lds<T>::floats() * 4 + norm_lds;
        break;
    }
    p.overlap = (p.family == F::Bf16BoxPi || p.family == F::F32Box) && !sw.cont_serial && terminal_obs_slots >= 2;
    p.grid = ceil_div(N, p.rows);
    return p;
}
inline RolloutPlan plan_rollout(int task, const PLayout &L, const tma_policy_dims &d, int64_t N, bool is_reset, int terminal_obs_slots, RolloutNorm norm,
                                const RolloutSwitches &sw) {
    RolloutPlan p;  // (an unknown task id: per-step, which refuses it)
    dispatch_task(task, [&](auto t) {
        p = plan_rollout_task<decltype(t)>(L, d, N, is_reset, terminal_obs_slots, norm, sw);
        return 0;
    });
    return p;
}

// tma_rollout_norm_plan: a view of the plan -- fused exactly where the step runs inside F32Disc's 8-env tiles or F32Box
inline int plan_rollout_norm(const RolloutPlan &p) {
    if (!p.norm_in_chunk) return TMA_ROLLOUT_NORM_PER_STEP;
    return p.family == RolloutFamily::F32Disc ? TMA_ROLLOUT_NORM_FUSED_DISC_F32 : TMA_ROLLOUT_NORM_FUSED_CONT_F32;
}
