// tma_ppo_types.h -- types shared by the translation units of the PPO update (tma_policy.hip, tma_h64.hip, ...); the workspace's layout and
// the capacities that size it are tma_workspace.h's.
#pragma once
#include "tma_workspace.h"

#include <cmath>

namespace tma {

// floats per packed sample record {obs padded to a multiple of 4 | log_prob, advantage, action bits, return}; 0: shape without them
static inline int rec_floats(const PLayout &L) { return (L.act == ACT_TANH && L.img_pi >= 0 && L.D <= 8) ? ((L.D + 3) & ~3) + 4 : 0; }

// What the bf16 column-parallel gradient launches for a shape (plan_grad_bf in tma_policy_plan.h decides, tma_launch_grad_wide_bf launches):
// ppo_grad_wide_bf_kernel<cont, H / 64, mt, kt1c, ks1c, PASS, waves>
enum class BfPass { Single, Cached, Recompute };  // one launch; PASS 0 + PASS 2 (dW1 from the dz1 cache); PASS 0 + PASS 1 (dW1 from a recomputed chain)
struct GradBfPlan {
    int32_t id;      // TMA_DISPATCH_GRAD_BF16_*
    int mt;          // 16-row tiles per row group: 2 or 4
    int waves;       // 4 (64 columns each) or 8 (32 columns each)
    int kt1c, ks1c;  // layer-1 k-tiles of dW1 in registers (single pass) / layer-1 k-steps (two passes); both 0: runtime width
    BfPass pass;
    int n_pi, n_vf;  // blocks = slabs of the policy net; the value net's blocks use the first n_vf of them
    int block, lds;  // threads, dynamic LDS bytes of every launch
    bool zero_w1;    // runtime width: dW1 accumulates in place in the slabs, behind slab_zero_w1_kernel
};

struct Minibatch {
    const int64_t *indices;  // optional explicit flat (env-major: f = i*T + t) indices
    uint32_t perm_seed, perm_epoch;
    int64_t start, count, total;  // rows [start, start+count) of the permuted buffer of `total` samples
    const int32_t *offs;          // optional: offs[j] = buffer offset of minibatch row j (written by adv_partial_kernel), saves the
                                  // permutation arithmetic in the gradient kernel
    int64_t stats_n;              // rows the advantage partials were summed over: count, or the global minibatch under data parallelism
    const double *adv_part;       // (sum, sum of squares) partials of this minibatch's advantages, adv_n_part pairs: kernels that fold the
    int adv_n_part;               // statistics themselves (H = 64, bf16 wide) read them; the others get (mean, std) from adv_final_kernel
};

__device__ __forceinline__ int64_t sample_offset(const Minibatch &mb, int64_t j, int T, int64_t N) {
    const int64_t f = mb.indices ? mb.indices[j] : (int64_t)perm_index(mb.perm_seed, mb.perm_epoch, (uint32_t)j, (uint32_t)mb.total);
    const int64_t i = f / T, t = f - i * T;  // swap_and_flatten: (T, N) -> env-major
    return t * N + i;
}

// ---- advantage pre-pass: sample offsets + (sum, sum of squares) partials of one minibatch ----
// Partial block `pb` of the `nb` a minibatch is split into: rows [pb * per, (pb + 1) * per) of it, thread tid < 256 takes rows j0 + tid,
// + 256, ... in that order into ONE f64 (sum, sum of squares) pair; one shuffle tree per wave, the four waves' pairs as (0 + 1) + (2 + 3).
// The ONE body of adv_partial_kernel (tma_policy.hip) and of the tail phase of the H = 64 gradient kernel's value blocks (tma_h64.hip),
// so the two cannot drift apart.  Four rows of a thread go through together -- four permutation evaluations, then four gathers in one
// memory round trip -- and are added in row order.  Every thread of the workgroup calls it (it holds a barrier); s1 / s2: 4 doubles of
// LDS each.  want_sums == false: offsets only (nothing reads the partials when advantages are not normalised), no barrier.
__device__ __forceinline__ void adv_partial_block(const float *__restrict__ adv, const Minibatch &mb, int T, int64_t N, int nb, int pb, int tid,
                                                  double *__restrict__ partials, int32_t *__restrict__ offs_out, bool want_sums, double *s1,
                                                  double *s2) {
    const int64_t per = (mb.count + nb - 1) / nb;
    const int64_t j0 = (int64_t)pb * per, j1 = (j0 + per < mb.count) ? j0 + per : mb.count;
    if (tid < 256) {
        double a = 0.0, b = 0.0;
        for (int64_t j = j0 + tid; j < j1; j += 4 * 256) {
            int64_t off[4];
            float x[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t jq = j + 256 * q;
                off[q] = 0;
                if (jq < j1) {
                    off[q] = sample_offset(mb, mb.start + jq, T, N);
                    if (offs_out) offs_out[jq] = (int32_t)off[q];
                }
            }
            if (want_sums) {
#pragma unroll
                for (int q = 0; q < 4; q++) x[q] = adv[off[q]];  // (rows past the slice read element 0 and are not added)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (j + 256 * q < j1) {
                        const double xd = (double)x[q];
                        a += xd;
                        b += xd * xd;
                    }
                }
            }
        }
        if (want_sums) {
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_down(a, o, 64);
                b += __shfl_down(b, o, 64);
            }
            if ((tid & 63) == 0) s1[tid >> 6] = a, s2[tid >> 6] = b;
        }
    }
    if (!want_sums) return;
    __syncthreads();
    if (tid == 0) {
        partials[2 * pb] = (s1[0] + s1[1]) + (s1[2] + s1[3]);
        partials[2 * pb + 1] = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    }
}

// The pre-pass of the NEXT minibatch, carried by an eight-wave H = 64 gradient launch (tma_ppo_train_epochs_local): value block b runs
// partial blocks b, b + n_pairs, ... of it after its own slab stores and statistics -- the value net's blocks finish ahead of the policy
// net's, so the launch does not grow -- and the next launch finds its offsets and partials where tma_ppo_epoch_prepare would have left
// them.  The kernel boundary is the hand-over; the regions written are never the ones the carrying launch reads.
struct PrepNext {
    const float *adv;             // the advantages plane [T][N]
    int32_t *offs_out;            // offs_out[j] = buffer offset of row j of that minibatch
    double *partials_out;         // its (sum, sum of squares) partials: Workspace::adv_stride(count) pairs; untouched without want_sums
    uint32_t perm_seed, perm_epoch;
    int64_t start, count, total;  // rows [start, start + count) of the (perm_seed, perm_epoch) permutation; count == 0: nothing to do
    int64_t N;
    int T;
    int want_sums;                // normalize_advantage; 0: offsets only
};

struct Rollout {
    const float *obs;
    const void *actions;
    const float *log_probs, *advantages, *returns;
    int T;
    int64_t N;
    const float *packed;  // optional sample records (tma_ppo_pack_samples), rec_floats(L) floats per sample
};
struct HParams {
    float clip_range, ent_coef, vf_coef;
    int normalize_advantage;
    int debug;  // TMA_BF_DEBUG (profiling aid, default 0): bit mask of phases the bf16 wide kernel skips -- timing attribution only
};

// A pending optimizer step applied in the PROLOGUE of the next H = 64 gradient launch (tma_ppo_train_epoch_local, round 3): instead of a
// separate clip + Adam launch between two minibatches, every workgroup of the next gradient kernel redoes the step for ITS net's 4 675
// parameters (adam_update_h64: the same routine, the same inputs, hence the same bits in every workgroup and as the optimizer launch) and
// builds its LDS weight image from the results instead of staging it from memory; workgroup 0 of each net writes the new state to the
// other half of a double buffer (the running launch still reads the old half).  grad == nullptr: no pending step, stage the image.
struct AdamFold {
    const float *grad;       // reduced gradient of the previous minibatch [P] (slab_reduce_kernel, overwrite mode)
    const double *sq_part;   // its sum-of-squares partials, one per 64 parameters
    int n_part;
    const float *p_cur, *m_cur, *v_cur;  // trainable parameters / Adam moments before the step
    float *p_nxt, *m_nxt, *v_nxt;        // ... and after it
    float max_norm, lr_step, beta1, beta2, bc2_sqrt, eps;  // (bc2_sqrt = sqrt(1 - beta2^t), lr_step = lr / (1 - beta1^t))
    double *norm_out;        // [2] total gradient norm, clip coefficient (statistics)
    float scale;             // factor on the gradient before the clip (1 on one GPU; 1 / world on the all-reduced SUM, tma_ppo_train_epoch_dp)
};

// The Adam arguments of an update driver, and the one place the bias-correction pair of a step is worked out (on the host, in double).
struct AdamArgs {
    float *exp_avg, *exp_avg_sq;
    double lr, beta1, beta2, eps, max_grad_norm;
    double grad_scale;  // factor on the gradient before the clip: 1 on one GPU, 1 / world on an all-reduced sum
    struct Step { float lr_step, bc2_sqrt; };  // lr / (1 - beta1^t), sqrt(1 - beta2^t)
    Step at(int64_t step) const {
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        return Step{(float)(lr / bc1), (float)sqrt(bc2)};
    }
};

// What every epoch driver of tma_policy.hip works on (the extern "C" entry points unpack their flat arguments into one of these, once)
struct EpochJob {
    float *params;
    const tma_policy_dims *d;
    PLayout L;
    const tma_rollout *rb;  // checked view (check_rollout_view); the kernels' Rollout is rollout_of(rb, ...)
    uint32_t perm_seed;
    int64_t batch_size;
    const tma_ppo_hparams *hp;
    float *grad;
    Workspace ws;
    hipStream_t s;
};

struct Net {
    const float *W1t, *b1, *W2t, *b2, *W3t, *b3, *W2, *W3;
};
__device__ __forceinline__ Net pi_net(const float *p, const PLayout &L) {
    return Net{p + L.pW1t, p + L.pb1, p + L.pW2t, p + L.pb2, p + L.pW3t, p + L.pb3, p + L.pW2, p + L.pW3};
}
__device__ __forceinline__ Net vf_net(const float *p, const PLayout &L) {
    return Net{p + L.vW1t, p + L.vb1, p + L.vW2t, p + L.vb2, p + L.vW3t, p + L.vb3, p + L.vW2, p + L.vW3};
}


struct LossStats {
    double a = 0.0, ent = 0.0, kl = 0.0, clip = 0.0, n = 0.0;
};

// clipped-surrogate + entropy gradient wrt the head outputs of one 16-row tile (C layout), written to dz3[16][ld3]
// RLO / RHI >= 0: the row range is a compile-time constant -- the rows of the range then form ONE basic block, and the scheduler interleaves
// their dependent chains (max / exp / sum / log / exp over DPP reductions: ~140 instructions a row, each waiting for the one before).  With
// the range in registers every row is a block of its own behind a wave-uniform branch and the chains run one after the other.
template <bool CONT, int RLO = -1, int RHI = -1>
__device__ __forceinline__ void policy_loss_tile(const f32x4 (&acc)[CONT ? 2 : 1], const float *meta, const int64_t *row_off, const void *actions,
                                                 const float *log_std, int A, float amean, float astd, const HParams &hp, float invB, float *dz3,
                                                 int ld3, float (&dlsd)[2], LossStats &st, int lane, int r_lo = 0, int r_hi = 4,
                                                 const float *act_tile = nullptr /* CONT: the tile's actions [16][32] in LDS (gathered with the observation rows, a phase ahead) instead of a global load here */) {
    const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if constexpr (RLO >= 0) {
            if (r < RLO || r >= RHI) continue;
        } else {
            if (r < r_lo || r >= r_hi) continue;  // (wave-uniform) a caller may split the four rows of a lane group over two waves
        }
        const int row = g * 4 + r;
        const int64_t off = row_off[row];
        const bool valid = off >= 0;
        const float old = meta[row * 4 + 0];
        const float advn = (meta[row * 4 + 1] - amean) / (astd + 1e-8f);
        float lpa, ent;
        float d[2] = {0.0f, 0.0f}, sd[2] = {1.0f, 1.0f}, p = 0.0f, lp = 0.0f;
        int act = 0;
        if constexpr (!CONT) {
            const bool colok = r16 < A;
            const float x = colok ? acc[0][r] : -INFINITY;
            const float m = gmax16(x);
            const float e = colok ? expf(x - m) : 0.0f;
            const float s = gsum16(e);
            const float lse = m + logf(s);
            lp = colok ? x - lse : 0.0f;
            p = e / s;
            act = __float_as_int(meta[row * 4 + 3]);
            lpa = gsum16((r16 == act) ? lp : 0.0f);
            ent = -gsum16(p * lp);
        } else {
            float lpsum = 0.0f, entsum = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int col = 16 * j + r16;
                if (col < A) {
                    const float lsd = log_std[col];
                    sd[j] = expf(lsd);
                    const float a = valid ? (act_tile ? act_tile[row * 32 + col] : static_cast<const float *>(actions)[off * A + col]) : 0.0f;
                    d[j] = a - acc[j][r];
                    lpsum += -(d[j] * d[j]) / (2.0f * (sd[j] * sd[j])) - lsd - 0.9189385332046727f;
                    entsum += 1.4189385332046727f + lsd;
                }
            }
            lpa = gsum16(lpsum);
            ent = gsum16(entsum);
        }
        const float ratio = expf(lpa - old);
        const float pl1 = advn * ratio;
        const float rc = fminf(fmaxf(ratio, 1.0f - hp.clip_range), 1.0f + hp.clip_range);
        const float pl2 = advn * rc;
        const float g_lp = (valid && pl1 <= pl2) ? -(advn * ratio) * invB : 0.0f;
        if constexpr (!CONT) {
            float dl = g_lp * (((r16 == act) ? 1.0f : 0.0f) - p);
            dl += valid ? (hp.ent_coef * invB) * (p * (lp + ent)) : 0.0f;
            dz3[row * ld3 + r16] = (r16 < A) ? dl : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int col = 16 * j + r16;
                const float var = sd[j] * sd[j];
                dz3[row * ld3 + col] = (col < A) ? g_lp * (d[j] / var) : 0.0f;
                if (col < A) dlsd[j] += g_lp * ((d[j] * d[j]) / var - 1.0f) - (valid ? hp.ent_coef * invB : 0.0f);
            }
        }
        // (selects instead of a divergent branch: adding +0.0 leaves a sum as it is, and the row stays one basic block)
        const bool on = valid && r16 == 0;
        st.a += on ? (double)(-fminf(pl1, pl2)) : 0.0;
        st.ent += on ? (double)ent : 0.0;
        st.kl += on ? (double)((ratio - 1.0f) - (lpa - old)) : 0.0;
        st.clip += (on && fabsf(ratio - 1.0f) > hp.clip_range) ? 1.0 : 0.0;
        st.n += on ? 1.0 : 0.0;
    }
}

// KT1C: k-tiles of dW1 kept in registers (1: D <= 16, 2: D <= 32), 0: layer-1 gradient accumulated in the slab, -1: dW1 skipped
// (first of two passes).  PASS 1 = second pass for wide observations of known width: the forward / backward chain is recomputed and
// ONLY dW1 (KT1C k-tiles) is accumulated and stored -- every other store is compiled out, so the MFMAs feeding only them vanish.
// NQ1C > 0: layer-1 weights (16 * NQ1C >= D rows) also run through the ring, from the fragment image PLayout::fr1_pi.
}  // namespace tma

// tma_h64.hip: the H = 64 persistent gradient kernel (internal, not part of the C ABI)
int tma_launch_grad_h64(const float *params, const tma::PLayout &L, const tma::Rollout &R, const tma::Minibatch &M, const tma::HParams &hpar,
                        const double *adv_part, int n_part, float *slabs, double *slots, int *n_slabs_out, hipStream_t s,
                        const tma::AdamFold *fold = nullptr, const tma::PrepNext *next = nullptr);
// true: a minibatch of `count` rows runs on the eight-wave kernel, whose value blocks can carry a PrepNext (and whose launch may be handed one)
bool tma_grad_h64_carries_prep(int64_t count);
int tma_h64_small_fold();  // TMA_H64_SMALL_SERIAL, read once per process: the FOLD mask of h64t_tile the H = 64 update kernels run

// tma_h64p.hip: `total` samples (whole epochs, prepared in job.ws) at batch_size = 256 as a single persistent launch (H = 64 fast-path layouts)
bool tma_epoch_h64p_eligible(const tma::PLayout &L, int64_t batch_size, int64_t total);
int tma_launch_epoch_h64p(const tma::EpochJob &job, const tma::Rollout &R, const tma::HParams &hp, int64_t total, int64_t first_step, const tma::AdamArgs &opt);

// tma_h256p.hip: the same for the reference's default 256 x 256 policy (exact f32, Discrete heads, observations <= 32): 2 x 32 workgroups on two XCDs
bool tma_epoch_h256p_eligible(const tma::PLayout &L, int64_t batch_size, int64_t total);
int tma_launch_epoch_h256p(const tma::EpochJob &job, const tma::Rollout &R, const tma::HParams &hp, int64_t total, int64_t first_step, const tma::AdamArgs &opt);

// tma_bf16.hip: the column-parallel bf16-MFMA gradient kernel (hidden 128 / 192 / 256) on the update workspace `ws` (advantage statistics,
// slabs, statistic slots, dz1 cache).  It launches what `plan` says (plan_grad_bf, tma_policy_plan.h) and decides nothing itself
int tma_launch_grad_wide_bf(const float *params, const tma::Rollout &R, const tma::Minibatch &M, const tma::HParams &hpar, const tma::Workspace &ws,
                            const tma::GradBfPlan &plan, hipStream_t s);
// tma_bf16.hip: the three-term bf16 split of the 256-wide f32 update (mfma_dtype = 2; tma_split3.h) and the rebuild of its weight planes
int tma_launch_grad_split3(const float *params, const tma::PLayout &L, const tma::Rollout &R, const tma::Minibatch &M, const tma::HParams &hpar, float *slabs,
                           double *slots, int *n_pi_out, int *n_vf_out, hipStream_t s);
int tma_launch_build_split3(float *params, const tma::PLayout &L, hipStream_t s);
bool tma_split3_eligible(const tma::PLayout &L, int64_t count);
// tma_policy.hip: zero the layer-1 weight columns of every slab (layouts that accumulate dW1 in place)
int tma_launch_slab_zero_w1(float *slabs, int n_slabs, const tma::PLayout &L, hipStream_t s);
// tma_policy.hip: the shape check every tma_policy_* entry point starts with (TMA_ERR_INVALID + message, no HIP call) -- for tma_vjp.hip
int tma_check_policy_dims(const tma_policy_dims *d);
