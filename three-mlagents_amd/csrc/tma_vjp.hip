// tma_vjp.hip -- vector-Jacobian product of tma_policy_evaluate_actions with respect to the trainable parameters (ABI 215):
//   grad[e] = sum_i  g_values[i] dV_i/dp_e + g_logp[i] dlogp_i/dp_e + g_entropy[i] dH_i/dp_e.
// What torch autograd does behind SB3's ActorCriticPolicy.evaluate_actions(obs, actions) when a user's own loss calls .backward() on it
// (behaviour cloning, distillation, KL penalties): the per-row coefficients come from the caller instead of from the PPO loss compiled into
// the gradient kernels of tma_policy.hip / tma_h64.hip / tma_bf16.hip, which this file leaves alone.
//
// DETERMINISTIC by construction: no float atomics.  The rows are walked in chunks; a chunk takes two launches.
//   (a) vjp_tile_kernel: one wave per 16-row tile and net -- forward (load_obs_tile, dense_act, dense_head), the head cotangent dz3 from the
//       three cotangent arrays, the input gradients dz2, dz1 (dense_bwd_input); h1, h2, dz1, dz2, dz3 (and the Box head's per-row log_std
//       terms) of the chunk go to the workspace, every row of every tile written (rows behind the batch carry dz = 0).
//   (b) vjp_reduce_kernel: the weight gradients as output-stationary GEMMs over the chunk's rows -- X^T dz1, h1^T dz2, h2^T dz3 -- and the bias
//       / log_std column sums as the same GEMM with a row of ones.  ONE workgroup owns an output tile (16 x 16 NTJ): its NW waves take the NW
//       contiguous segments of the chunk's k-steps (four rows each, in row order: a k-ordered fmaf chain per wave), the NW partial tiles are
//       added in segment order through LDS, and the owner adds the result to grad_out with a plain load-add-store (chunk 0 stores).
// Summation order of one gradient element: rows in order inside a segment, segments in order inside a chunk, chunks in order.  It depends on
// (shape, n, chunk length) and on nothing else, so equal inputs give equal bits.
// Both kernels are bounded loops over their own rows: no spin waits, no exchange between workgroups.
//   (c) vjp_input_kernel (ABI 222, only where the caller asks for grad_obs): the gradient with respect to the observations of the chunk's rows,
//       dObs[i][k] = sum_n dz1_pi[i][n] W1t_pi[k][n] + sum_n dz1_vf[i][n] W1t_vf[k][n], from the two dz1 planes phase (a) left behind.  One wave per
//       16-row tile, no reduction over rows, plain stores: rows [base, base + rows) of grad_obs are overwritten.  Where grad_params is not asked
//       for (a frozen policy) phase (b) is not launched: (a) then (c) per chunk.
//
// tma_policy_head_backward (ABI 218) is the same two launches for the head itself (tma_policy_head: logits / mean, and values):
//   grad[e] = sum_i sum_j g_head[i][j] dhead_ij/dp_e + sum_i g_values[i] dV_i/dp_e.
// Phase (a) takes dz3 of a policy row straight from g_head's row (vjp_tile_body<.., HEAD>); phase (b) is the code above, unchanged, and its
// log_std job sums a plane of zeros.
#include "tma_ppo_types.h"

#include <cstdlib>

namespace tma {

constexpr int VJP_LD3 = 32;              // row stride of the dz3 / log_std planes (heads have at most 32 columns; the columns behind the head are zero)
constexpr int64_t VJP_MAX_CHUNK = 16384;  // rows per chunk at the most ...
constexpr int64_t VJP_WS_TARGET = 128ll << 20;  // ... and as many as keep the planes within this (the bound tma.h promises is 256 MB)
constexpr int VJP_LDS_LIMIT = 160 * 1024, VJP_LDS_OPT_IN = 64 * 1024;

// planes of one chunk in the workspace: cap rows each
struct VjpPlanes {
    float *h1[2], *h2[2], *dz1[2], *dz2[2], *dz3[2];  // [net: 0 policy, 1 value]; h*, dz1, dz2: [cap][H], dz3: [cap][VJP_LD3]
    float *dls;                                       // [cap][VJP_LD3]: per-row terms of the log_std gradient (Box heads)
};

static inline int64_t vjp_row_floats(const PLayout &L) { return 8 * (int64_t)L.H + 3 * VJP_LD3; }
static inline int64_t vjp_default_chunk(const PLayout &L) {
    int64_t c = (VJP_WS_TARGET / (vjp_row_floats(L) * 4)) & ~(int64_t)15;
    return c > VJP_MAX_CHUNK ? VJP_MAX_CHUNK : c;
}
__host__ __device__ inline int vjp_tile_lds_floats(const PLayout &L) {
    const int ldx = ((L.D + 3) & ~3) + 2, ld = L.H + 2;
    return 16 * (ldx + 2 * ld + (VJP_LD3 + 2)) + 16 * 2 + 16 * 4;  // X, h1, h2, dz3, row_off (int64), meta
}

// coalesced copy of a wave's [16][cols] LDS tile (row stride ld) to rows [row0, row0 + 16) of a [cap][cols] plane
__device__ __forceinline__ void store_tile(const float *t, int ld, int cols, float *plane, int row0, int lane) {
    float *dst = plane + (int64_t)row0 * cols;
    for (int e = lane; e < 16 * cols; e += 64) {
        const int row = e / cols, c = e - row * cols;
        dst[e] = t[row * ld + c];
    }
}

// ---- (a) one wave per tile: forward, head cotangent, input gradients -> planes
// HEAD (tma_policy_head_backward, ABI 218): the head cotangent is the caller's -- `g_logp` carries g_head f32[n][A] (or null), `actions` and
// `g_entropy` are not read, the head's forward is not needed, and the Box head's log_std plane is zeros (the head does not depend on log_std)
template <bool CONT, bool IS_PI, bool HEAD, int ACT>
__device__ __forceinline__ void vjp_tile_body(const float *__restrict__ params, const PLayout &L, const float *__restrict__ obs,
                                              const void *__restrict__ actions, int64_t row_base, int rows, const float *__restrict__ g_values,
                                              const float *__restrict__ g_logp, const float *__restrict__ g_entropy, const VjpPlanes &ws, float *smem) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int D = L.D, H = L.H, A = L.A;
    const int ldx = ((D + 3) & ~3) + 2, ld = H + 2, ld3 = VJP_LD3 + 2;
    float *X = smem + (int64_t)wave * vjp_tile_lds_floats(L);
    float *h1 = X + 16 * ldx, *h2 = h1 + 16 * ld, *dzA = h2, *dzB = h1, *dz3 = h2 + 16 * ld;
    int64_t *row_off = reinterpret_cast<int64_t *>(dz3 + 16 * ld3);
    float *meta = reinterpret_cast<float *>(row_off + 16);  // [16][4]: g_logp, g_entropy, action bits, g_values
    const Net Q = IS_PI ? pi_net(params, L) : vf_net(params, L);
    const int NOUT = IS_PI ? A : 1, net = IS_PI ? 0 : 1;
    const int n_tiles = (rows + 15) >> 4;
    for (int tile = blockIdx.x * wpb + wave; tile < n_tiles; tile += gridDim.x * wpb) {
        const int row0 = tile << 4;
        if (lane < 16) {
            const bool valid = row0 + lane < rows;
            const int64_t grow = row_base + row0 + lane;
            row_off[lane] = valid ? grow : -1;
            meta[lane * 4 + 0] = (!HEAD && valid && g_logp != nullptr) ? g_logp[grow] : 0.0f;
            meta[lane * 4 + 1] = (!HEAD && valid && g_entropy != nullptr) ? g_entropy[grow] : 0.0f;
            meta[lane * 4 + 2] = (!HEAD && !CONT && IS_PI && valid) ? __int_as_float(static_cast<const int32_t *>(actions)[grow]) : 0.0f;
            meta[lane * 4 + 3] = (valid && g_values != nullptr) ? g_values[grow] : 0.0f;
        }
        load_obs_tile(obs, row_off, D, X, ldx, lane);
        dense_act<ACT>(X, ldx, D, Q.W1t, Q.b1, H, h1, ld, lane);
        store_tile(h1, ld, H, ws.h1[net], row0, lane);
        dense_act<ACT>(h1, ld, H, Q.W2t, Q.b2, H, h2, ld, lane);
        store_tile(h2, ld, H, ws.h2[net], row0, lane);
        if constexpr (!IS_PI) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = g * 4 + r;
                dz3[row * ld3 + r16] = r16 == 0 ? meta[row * 4 + 3] : 0.0f;  // dV/dz3 = 1
                dz3[row * ld3 + 16 + r16] = 0.0f;
            }
        } else if constexpr (HEAD) {
            const float *g_head = g_logp;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = g * 4 + r;
                const int64_t off = row_off[row];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int col = 16 * j + r16;
                    dz3[row * ld3 + col] = (g_head != nullptr && off >= 0 && col < A) ? g_head[off * A + col] : 0.0f;
                    if constexpr (CONT) ws.dls[(int64_t)(row0 + row) * VJP_LD3 + col] = 0.0f;
                }
            }
        } else if constexpr (!CONT) {
            f32x4 acc[1];
            dense_head<1>(h2, ld, H, Q.W3t, Q.b3, A, acc, lane);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = g * 4 + r;
                const bool colok = r16 < A;
                const float x = colok ? acc[0][r] : -INFINITY;
                const float m = gmax16(x);
                const float e = colok ? expf(x - m) : 0.0f;
                const float s = gsum16(e);
                const float lse = m + logf(s);
                const float lp = colok ? x - lse : 0.0f;
                const float p = e / s;
                const int act = __float_as_int(meta[row * 4 + 2]);  // only ever compared with a column index
                const float ent = -gsum16(p * lp);
                const float g_lp = meta[row * 4 + 0], g_ent = meta[row * 4 + 1];
                // a zero cotangent contributes an exact +0 whatever the action (so a row whose g_logp is 0 does not depend on its action at all)
                const float t_lp = g_lp != 0.0f ? g_lp * (((r16 == act) ? 1.0f : 0.0f) - p) : 0.0f;
                const float t_ent = g_ent != 0.0f ? g_ent * (p * (lp + ent)) : 0.0f;
                dz3[row * ld3 + r16] = colok ? t_lp - t_ent : 0.0f;
                dz3[row * ld3 + 16 + r16] = 0.0f;
            }
        } else {
            f32x4 acc[2];
            dense_head<2>(h2, ld, H, Q.W3t, Q.b3, A, acc, lane);
            const float *lsp = params + L.log_std;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = g * 4 + r;
                const int64_t off = row_off[row];
                const float g_lp = meta[row * 4 + 0], g_ent = meta[row * 4 + 1];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int col = 16 * j + r16;
                    float dm = 0.0f, dl = 0.0f;
                    if (col < A) {
                        const float sd = expf(lsp[col]), var = sd * sd;
                        const float a = off >= 0 ? static_cast<const float *>(actions)[off * A + col] : 0.0f;
                        const float d = a - acc[j][r];
                        dm = g_lp * (d / var);
                        dl = g_lp * ((d * d) / var - 1.0f) + g_ent;
                    }
                    dz3[row * ld3 + col] = dm;
                    ws.dls[(int64_t)(row0 + row) * VJP_LD3 + col] = dl;
                }
            }
        }
        store_tile(dz3, ld3, VJP_LD3, ws.dz3[net], row0, lane);
        dense_bwd_input<ACT>(dz3, ld3, NOUT, Q.W3, H, h2, ld, dzA, ld, lane);
        store_tile(dzA, ld, H, ws.dz2[net], row0, lane);
        dense_bwd_input<ACT>(dzA, ld, H, Q.W2, H, h1, ld, dzB, ld, lane);
        store_tile(dzB, ld, H, ws.dz1[net], row0, lane);
    }
}

// grid (tile blocks, 2): blockIdx.y = 0 the policy net, 1 the value net
template <bool CONT, bool HEAD, int ACT>
__global__ __launch_bounds__(256) void vjp_tile_kernel(const float *__restrict__ params, PLayout L, const float *__restrict__ obs,
                                                       const void *__restrict__ actions, int64_t row_base, int rows,
                                                       const float *__restrict__ g_values, const float *__restrict__ g_logp,
                                                       const float *__restrict__ g_entropy, VjpPlanes ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (blockIdx.y == 0) vjp_tile_body<CONT, true, HEAD, ACT>(params, L, obs, actions, row_base, rows, g_values, g_logp, g_entropy, ws, smem);
    else vjp_tile_body<CONT, false, HEAD, ACT>(params, L, obs, actions, row_base, rows, g_values, g_logp, g_entropy, ws, smem);
}

// ---- (b) output-stationary weight-gradient GEMMs.  Jobs of one net, in block order:
//   W1: obs^T dz1 [D][H] | b1: 1^T dz1 | W2: h1^T dz2 [H][H] | b2 | W3: h2^T dz3 [H][n_out] | b3 | log_std: 1^T dls (policy net of a Box head)
// Every job is out[K][N] (+)= A[rows][K]^T B[rows][N]; a bias job has K = 1 and A = ones.  Tiles are 16 rows x 16 NTJ columns.
struct VjpJob {
    const float *A, *B;  // A == nullptr: ones
    float *out;
    int K, N, lda, ldb, ldo, a_rows;  // a_rows: rows of A that exist (the observations end with the batch; the planes are written to the tile)
    int k0, n0;
};

template <int NTJ>
__host__ __device__ inline int vjp_net_tiles(const PLayout &L, int net) {
    const int CW = 16 * NTJ, hk = L.H / 16, hn = (L.H + CW - 1) / CW, n_out = net == 0 ? L.A : 1, on = (n_out + CW - 1) / CW;
    return ((L.D + 15) / 16) * hn + hn + hk * hn + hn + hk * on + on + ((net == 0 && L.cont) ? on : 0);
}

template <int NTJ>
__device__ __forceinline__ VjpJob vjp_job(const PLayout &L, const VjpPlanes &ws, const float *obs_chunk, int rows, float *grad, int b) {
    constexpr int CW = 16 * NTJ;
    const int t0 = vjp_net_tiles<NTJ>(L, 0);
    const int net = b < t0 ? 0 : 1;
    int x = net == 0 ? b : b - t0;
    const int D = L.D, H = L.H, n_out = net == 0 ? L.A : 1;
    const int hk = H / 16, hn = (H + CW - 1) / CW, on = (n_out + CW - 1) / CW, dk = (D + 15) / 16;
    const int oW1 = net == 0 ? L.pW1t : L.vW1t, ob1 = net == 0 ? L.pb1 : L.vb1, oW2 = net == 0 ? L.pW2t : L.vW2t, ob2 = net == 0 ? L.pb2 : L.vb2;
    const int oW3 = net == 0 ? L.pW3t : L.vW3t, ob3 = net == 0 ? L.pb3 : L.vb3;
    const int rows16 = (rows + 15) & ~15;
    if (x < dk * hn) return VjpJob{obs_chunk, ws.dz1[net], grad + oW1, D, H, D, H, H, rows, 16 * (x / hn), CW * (x % hn)};
    x -= dk * hn;
    if (x < hn) return VjpJob{nullptr, ws.dz1[net], grad + ob1, 1, H, 0, H, H, rows16, 0, CW * x};
    x -= hn;
    if (x < hk * hn) return VjpJob{ws.h1[net], ws.dz2[net], grad + oW2, H, H, H, H, H, rows16, 16 * (x / hn), CW * (x % hn)};
    x -= hk * hn;
    if (x < hn) return VjpJob{nullptr, ws.dz2[net], grad + ob2, 1, H, 0, H, H, rows16, 0, CW * x};
    x -= hn;
    if (x < hk * on) return VjpJob{ws.h2[net], ws.dz3[net], grad + oW3, H, n_out, H, VJP_LD3, n_out, rows16, 16 * (x / on), CW * (x % on)};
    x -= hk * on;
    if (x < on) return VjpJob{nullptr, ws.dz3[net], grad + ob3, 1, n_out, 0, VJP_LD3, n_out, rows16, 0, CW * x};
    x -= on;
    return VjpJob{nullptr, ws.dls, grad + L.log_std, 1, n_out, 0, VJP_LD3, n_out, rows16, 0, CW * x};
}

template <int NTJ, int NW>
__global__ __launch_bounds__(64 * NW) void vjp_reduce_kernel(PLayout L, VjpPlanes ws, const float *__restrict__ obs_chunk, int rows,
                                                             float *__restrict__ grad, int accumulate) {
    constexpr int CW = 16 * NTJ, KB = NTJ == 1 ? 32 : 16;  // k-steps per batch of loads: every load of a batch in flight together, then its MFMAs
    __shared__ float part[NW][16][CW + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const VjpJob J = vjp_job<NTJ>(L, ws, obs_chunk, rows, grad, (int)blockIdx.x);
    const int krow = J.k0 + r16;
    const bool a_ok = krow < J.K;
    const float *Ap = J.A != nullptr ? J.A + krow : nullptr;
    bool b_ok[NTJ];
    const float *Bp[NTJ];
#pragma unroll
    for (int j = 0; j < NTJ; j++) {
        const int col = J.n0 + 16 * j + r16;
        b_ok[j] = col < J.ldb;  // (columns in [N, ldb) of a head plane are stored zeros)
        Bp[j] = J.B + (b_ok[j] ? col : 0);
    }
    f32x4 acc[NTJ];
#pragma unroll
    for (int j = 0; j < NTJ; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int nq = ((rows + 15) & ~15) >> 2, per = (nq + NW - 1) / NW;  // k-steps of four rows; this wave's are [wave per, min(nq, (wave + 1) per))
    const int q_beg = wave * per, q_end = (wave + 1) * per < nq ? (wave + 1) * per : nq;
    for (int q0 = q_beg; q0 < q_end; q0 += KB) {
        float a[KB], b[KB][NTJ];
#pragma unroll
        for (int v = 0; v < KB; v++) {
            const bool in = q0 + v < q_end;
            const int row = 4 * (in ? q0 + v : q_beg) + g;
            a[v] = !in ? 0.0f : (Ap == nullptr ? 1.0f : ((a_ok && row < J.a_rows) ? Ap[(int64_t)row * J.lda] : 0.0f));
#pragma unroll
            for (int j = 0; j < NTJ; j++) b[v][j] = (in && b_ok[j]) ? Bp[j][(int64_t)row * J.ldb] : 0.0f;
        }
#pragma unroll
        for (int v = 0; v < KB; v++)
#pragma unroll
            for (int j = 0; j < NTJ; j++) acc[j] = mfma16(a[v], b[v][j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NTJ; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) part[wave][4 * g + r][16 * j + r16] = acc[j][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * CW; e += 64 * NW) {  // the owner of the tile folds the segments in order
        const int i = e / CW, c = e - i * CW;
        float tot = part[0][i][c];
#pragma unroll
        for (int w = 1; w < NW; w++) tot += part[w][i][c];
        const int k = J.k0 + i, col = J.n0 + c;
        if (k < J.K && col < J.N) {
            float *dst = J.out + (int64_t)k * J.ldo + col;
            *dst = accumulate ? *dst + tot : tot;
        }
    }
}

// ---- (c) the observation gradient of a chunk: dObs[16][D] = dz1_pi[16][H] . W1t_pi[D][H]^T + dz1_vf[16][H] . W1t_vf[D][H]^T
// No [out][in] copy of W1 exists and none is needed: the B operand of output column k and products n is W1t[k][n], so the four n a lane feeds to
// four consecutive k-steps are 16 contiguous bytes of row k -- and the A operand the same 16 bytes of the dz1 row.  Both come straight from
// global memory (W1t is at most 172 x 1024 floats per net and L2-resident; a dz1 tile is read once per pass of 64 columns, and the
// passes of a tile are separate waves), no LDS.
// The value net's W1t starts at an odd float offset for most heads, hence the 4-byte-aligned vector type (gfx950 loads it as one dwordx4).
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// NT column tiles [k0, k0 + 16 NT) of one row tile.  ONE accumulator chain per output element: the policy net's H products, then the value net's,
// each net in blocks of 16 n (q), inside a block k-step v = 0..3 takes n = 16 q + 4 g + v from lane group g = 0..3 (the MFMA's own k order) --
// a fixed order that depends on nothing but H, so equal inputs give equal bits whatever the batch, the chunk length or the row's place in it.
// Columns k >= D read row D - 1 (an address that exists) and are never stored: an MFMA column depends on its own B column alone.
template <int NT>
__device__ __forceinline__ void vjp_input_pass(const float *a_pi, const float *a_vf, const float *__restrict__ w_pi, const float *__restrict__ w_vf, int H,
                                               int D, int k0, float *__restrict__ out, int rows_left, int lane) {
    constexpr int QB = NT <= 2 ? 4 : 2;  // blocks of 16 n per batch of loads (H % 64 == 0: H / 16 is a multiple of 4)
    const int r16 = lane & 15, g = lane >> 4;
    int woff[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int k = k0 + 16 * j + r16;
        woff[j] = (k < D ? k : D - 1) * H + 4 * g;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int net = 0; net < 2; net++) {
        const float *a = (net == 0 ? a_pi : a_vf) + r16 * H + 4 * g;
        const float *w = net == 0 ? w_pi : w_vf;
        for (int q0 = 0; q0 < (H >> 4); q0 += QB) {
            f32x4 av[QB], bv[QB][NT];
#pragma unroll
            for (int u = 0; u < QB; u++) {
                av[u] = *reinterpret_cast<const f32x4 *>(a + 16 * (q0 + u));
#pragma unroll
                for (int j = 0; j < NT; j++) bv[u][j] = *reinterpret_cast<const f32x4_a4 *>(w + woff[j] + 16 * (q0 + u));
            }
#pragma unroll
            for (int u = 0; u < QB; u++)
#pragma unroll
                for (int v = 0; v < 4; v++)
#pragma unroll
                    for (int j = 0; j < NT; j++) acc[j] = mfma16(av[u][v], bv[u][j][v], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int col = k0 + 16 * j + r16;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = g * 4 + r;
            if (row < rows_left && col < D) out[(int64_t)row * D + col] = acc[j][r];  // rows behind the batch are not stored
        }
    }
}

// grid (16-row tiles of the chunk, passes of 64 output columns): one wave each.  The row index into a dz1 plane is chunk-local, the one into
// grad_obs global (64-bit)
__global__ __launch_bounds__(64) void vjp_input_kernel(const float *__restrict__ params, PLayout L, VjpPlanes ws, int64_t row_base, int rows,
                                                       float *__restrict__ grad_obs) {
    const int lane = threadIdx.x, row0 = (int)blockIdx.x << 4, ct = (int)blockIdx.y << 2;
    const int D = L.D, H = L.H, n_ct = (D + 15) >> 4;  // column tiles of 16; this wave's are [ct, min(ct + 4, n_ct))
    if (row0 >= rows || ct >= n_ct) return;
    const float *a_pi = ws.dz1[0] + (int64_t)row0 * H, *a_vf = ws.dz1[1] + (int64_t)row0 * H;
    const float *w_pi = params + L.pW1t, *w_vf = params + L.vW1t;
    float *out = grad_obs + (row_base + row0) * D;
    const int left = rows - row0;
    switch (n_ct - ct) {
    case 1: vjp_input_pass<1>(a_pi, a_vf, w_pi, w_vf, H, D, 16 * ct, out, left, lane); break;
    case 2: vjp_input_pass<2>(a_pi, a_vf, w_pi, w_vf, H, D, 16 * ct, out, left, lane); break;
    case 3: vjp_input_pass<3>(a_pi, a_vf, w_pi, w_vf, H, D, 16 * ct, out, left, lane); break;
    default: vjp_input_pass<4>(a_pi, a_vf, w_pi, w_vf, H, D, 16 * ct, out, left, lane); break;
    }
}

static int vjp_chunk_rows(const PLayout &L, int64_t *out) {
    int64_t c = vjp_default_chunk(L);
    if (const char *e = getenv("TMA_VJP_CHUNK_ROWS"); e && *e) {  // test hook, read on every call: shorter chunks (never longer: the workspace is sized for the default)
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (*end != '\0' || v < 16 || v % 16 != 0) return fail(TMA_ERR_INVALID, "TMA_VJP_CHUNK_ROWS must be a multiple of 16, at least 16 (got '%s')", e);
        if (v < c) c = v;
    }
    *out = c;
    return TMA_OK;
}

}  // namespace tma

using namespace tma;

static int vjp_check(const tma_policy_dims *d, const char *who) {
    const int rc = tma_check_policy_dims(d);
    if (rc) return rc;
    if (d->mfma_dtype == 1)
        return fail(TMA_ERR_INVALID, "%s: mfma_dtype 1 (bf16) is not supported -- its forward rounds the operands to bf16 and an f32 backward would not be its derivative",
                    who);
    return TMA_OK;
}

extern "C" {

int64_t tma_policy_vjp_workspace_bytes(const tma_policy_dims *d, int64_t n) {
    if (vjp_check(d, "tma_policy_vjp_workspace_bytes")) return 0;
    if (n < 1) {
        fail(TMA_ERR_INVALID, "tma_policy_vjp_workspace_bytes: n must be >= 1");
        return 0;
    }
    const PLayout L = make_layout(d->obs_dim, d->hidden, d->act_dim, d->continuous, d->mfma_dtype, d->activation);
    const int64_t chunk = vjp_default_chunk(L), n16 = (n + 15) & ~(int64_t)15;
    return (n16 < chunk ? n16 : chunk) * vjp_row_floats(L) * 4;
}

}  // extern "C"

static bool bytes_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// every entry point behind its own null checks.  head: g_logp carries g_head f32[n][act_dim], actions / g_entropy are null.  grad_out
// (parameters) and grad_obs may each be null, not both: without grad_out phase (b) is not launched, without grad_obs phase (c)
static int vjp_run(const char *who, bool head, const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                   const float *g_values, const float *g_logp, const float *g_entropy, float *grad_out, float *grad_obs, void *workspace,
                   int64_t workspace_bytes, void *stream) {
    int rc = TMA_OK;
    const int64_t need = tma_policy_vjp_workspace_bytes(d, n);
    if (!workspace || workspace_bytes < need)
        return fail(TMA_ERR_INVALID, "%s: workspace of %lld bytes, tma_policy_vjp_workspace_bytes reports %lld", who, (long long)(workspace ? workspace_bytes : 0),
                    (long long)need);
    if (grad_obs && bytes_overlap(grad_obs, n * d->obs_dim * 4, workspace, workspace_bytes))
        return fail(TMA_ERR_INVALID, "%s: grad_obs overlaps the workspace", who);
    const PLayout L = make_layout(d->obs_dim, d->hidden, d->act_dim, d->continuous, d->mfma_dtype, d->activation);
    int64_t chunk = 0;
    if ((rc = vjp_chunk_rows(L, &chunk))) return rc;
    const int lds1 = vjp_tile_lds_floats(L) * 4;
    if (lds1 > VJP_LDS_LIMIT)
        return fail(TMA_ERR_INVALID, "%s: policy too wide for the LDS-resident tile (obs_dim %d, hidden %d: needs %d bytes)", who, L.D, L.H, lds1);
    if (d->device >= 0) {
        int cur = -1;
        TMA_HIP(hipGetDevice(&cur));
        if (cur != d->device) TMA_HIP(hipSetDevice(d->device));
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n16 = (n + 15) & ~(int64_t)15;
    const int64_t cap = n16 < chunk ? n16 : chunk;  // rows of a plane
    VjpPlanes ws;
    {
        float *p = static_cast<float *>(workspace);
        for (int net = 0; net < 2; net++) {
            ws.h1[net] = p, p += cap * L.H;
            ws.h2[net] = p, p += cap * L.H;
            ws.dz1[net] = p, p += cap * L.H;
            ws.dz2[net] = p, p += cap * L.H;
            ws.dz3[net] = p, p += cap * VJP_LD3;
        }
        ws.dls = p;
    }
    const bool wide = L.H > 64;  // 16 x 64 tiles on eight row segments; H = 64: 16 x 16 tiles on sixteen (few tiles, little traffic: parallelism over rows)
    const int n_blocks = wide ? vjp_net_tiles<4>(L, 0) + vjp_net_tiles<4>(L, 1) : vjp_net_tiles<1>(L, 0) + vjp_net_tiles<1>(L, 1);
    for (int64_t base = 0; base < n; base += chunk) {
        const int rows = (int)(n - base < chunk ? n - base : chunk);
        const int tiles = (rows + 15) >> 4;
        int wpb = tiles >= 1024 ? 4 : 1;  // small chunks: one wave per block so every CU gets work
        while (wpb > 1 && wpb * lds1 > VJP_LDS_LIMIT) wpb >>= 1;
        const int lds = wpb * lds1;
        auto launch_a = [&](auto k) -> int {
            if (lds > VJP_LDS_OPT_IN) TMA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            k<<<dim3((unsigned)((tiles + wpb - 1) / wpb), 2), dim3(64 * wpb), lds, s>>>(params, L, obs, actions, base, rows, g_values, g_logp, g_entropy, ws);
            TMA_LAUNCH_CHECK();
            return TMA_OK;
        };
        if (L.act == ACT_RELU) {
            if (head) rc = L.cont ? launch_a(vjp_tile_kernel<true, true, ACT_RELU>) : launch_a(vjp_tile_kernel<false, true, ACT_RELU>);
            else rc = L.cont ? launch_a(vjp_tile_kernel<true, false, ACT_RELU>) : launch_a(vjp_tile_kernel<false, false, ACT_RELU>);
        } else if (head) rc = L.cont ? launch_a(vjp_tile_kernel<true, true, ACT_TANH>) : launch_a(vjp_tile_kernel<false, true, ACT_TANH>);
        else rc = L.cont ? launch_a(vjp_tile_kernel<true, false, ACT_TANH>) : launch_a(vjp_tile_kernel<false, false, ACT_TANH>);
        if (rc) return rc;
        if (grad_out) {
            const float *obs_chunk = obs + base * L.D;
            if (wide) vjp_reduce_kernel<4, 8><<<dim3((unsigned)n_blocks), dim3(512), 0, s>>>(L, ws, obs_chunk, rows, grad_out, base > 0 ? 1 : 0);
            else vjp_reduce_kernel<1, 16><<<dim3((unsigned)n_blocks), dim3(1024), 0, s>>>(L, ws, obs_chunk, rows, grad_out, base > 0 ? 1 : 0);
            TMA_LAUNCH_CHECK();
        }
        if (grad_obs) {
            vjp_input_kernel<<<dim3((unsigned)tiles, (unsigned)((L.D + 63) / 64)), dim3(64), 0, s>>>(params, L, ws, base, rows, grad_obs);
            TMA_LAUNCH_CHECK();
        }
    }
    return TMA_OK;
}

// the refusals of the four entry points, in one order: dims, null inputs, n, cotangents, outputs, overlap with obs (then vjp_run's: workspace)
static int vjp_eval(const char *who, const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                    const float *g_values, const float *g_logp, const float *g_entropy, float *grad_params, float *grad_obs, bool params_required,
                    void *workspace, int64_t workspace_bytes, void *stream) {
    const int rc = vjp_check(d, who);  // (every refusal comes back before the first HIP call)
    if (rc) return rc;
    if (!params || !obs || !actions || (params_required && !grad_params)) return fail(TMA_ERR_INVALID, "%s: null buffer", who);
    if (n < 1) return fail(TMA_ERR_INVALID, "%s: n must be >= 1", who);
    if (!g_values && !g_logp && !g_entropy) return fail(TMA_ERR_INVALID, "%s: g_values, g_logp and g_entropy are all null", who);
    if (!grad_params && !grad_obs) return fail(TMA_ERR_INVALID, "%s: grad_params and grad_obs are both null", who);
    if (grad_obs && bytes_overlap(grad_obs, n * d->obs_dim * 4, obs, n * d->obs_dim * 4)) return fail(TMA_ERR_INVALID, "%s: grad_obs overlaps obs", who);
    return vjp_run(who, false, params, d, obs, actions, n, g_values, g_logp, g_entropy, grad_params, grad_obs, workspace, workspace_bytes, stream);
}

static int vjp_head(const char *who, const float *params, const tma_policy_dims *d, const float *obs, int64_t n, const float *g_head,
                    const float *g_values, float *grad_params, float *grad_obs, bool params_required, void *workspace, int64_t workspace_bytes,
                    void *stream) {
    const int rc = vjp_check(d, who);
    if (rc) return rc;
    if (!params || !obs || (params_required && !grad_params)) return fail(TMA_ERR_INVALID, "%s: null buffer", who);
    if (n < 1) return fail(TMA_ERR_INVALID, "%s: n must be >= 1", who);
    if (!g_head && !g_values) return fail(TMA_ERR_INVALID, "%s: g_head and g_values are both null", who);
    if (!grad_params && !grad_obs) return fail(TMA_ERR_INVALID, "%s: grad_params and grad_obs are both null", who);
    if (grad_obs && bytes_overlap(grad_obs, n * d->obs_dim * 4, obs, n * d->obs_dim * 4)) return fail(TMA_ERR_INVALID, "%s: grad_obs overlaps obs", who);
    return vjp_run(who, true, params, d, obs, nullptr, n, g_values, g_head, nullptr, grad_params, grad_obs, workspace, workspace_bytes, stream);
}

extern "C" {

int tma_policy_evaluate_actions_backward(const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                                         const float *g_values, const float *g_logp, const float *g_entropy, float *grad_out, void *workspace,
                                         int64_t workspace_bytes, void *stream) {
    return vjp_eval("tma_policy_evaluate_actions_backward", params, d, obs, actions, n, g_values, g_logp, g_entropy, grad_out, nullptr, true, workspace,
                    workspace_bytes, stream);
}

int tma_policy_evaluate_actions_vjp(const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n,
                                    const float *g_values, const float *g_logp, const float *g_entropy, float *grad_params, float *grad_obs,
                                    void *workspace, int64_t workspace_bytes, void *stream) {
    return vjp_eval("tma_policy_evaluate_actions_vjp", params, d, obs, actions, n, g_values, g_logp, g_entropy, grad_params, grad_obs, false, workspace,
                    workspace_bytes, stream);
}

int tma_policy_head_backward(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, const float *g_head, const float *g_values,
                             float *grad_out, void *workspace, int64_t workspace_bytes, void *stream) {
    return vjp_head("tma_policy_head_backward", params, d, obs, n, g_head, g_values, grad_out, nullptr, true, workspace, workspace_bytes, stream);
}

int tma_policy_head_vjp(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, const float *g_head, const float *g_values,
                        float *grad_params, float *grad_obs, void *workspace, int64_t workspace_bytes, void *stream) {
    return vjp_head("tma_policy_head_vjp", params, d, obs, n, g_head, g_values, grad_params, grad_obs, false, workspace, workspace_bytes, stream);
}

}  // extern "C"
