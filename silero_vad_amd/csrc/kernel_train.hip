// kernel_train.hip -- loss and gradients of the decoder by back-propagation through time (reference train(), tuning/utils.py:206-249;
// the rule and the workspace are trainer.hpp), and the unpack step of vad_encode_audio.
//
//   train_gates_kernel     GX[N][512] = feat W_ih^T + (b_ih + b_hh), N = B T: fp32 MFMA (v_mfma_f32_16x16x4_f32).  A wave holds the
//                          K = 128 fragment of 16 chunks in 32 registers and walks the 32 tiles of gate rows.
//   train_forward_kernel   the recurrence with the parameters of THIS call: one workgroup of 512 threads per row, thread j owns gate
//                          row j with its W_hh row in 128 registers, h broadcast from LDS, two barriers a step.  It keeps the four
//                          activated gates, c, tanh c and h per chunk, and wave 0 runs the head one step behind: p, the loss term (the
//                          row's sum in double, in chunk order), dz.
//   train_backward_kernel  walks t downwards, the same shape: thread (q, k) owns the 128 weights W_hh[128 q + u][k] and adds its share
//                          of W_hh^T dG_{t+1}; threads k < 128 fold the four shares and form dc and the four dG of their unit.
//   train_wgrad_kernel     dG^T feat and dG^T H_prev as split-K MFMA GEMMs over N, each split into its own slab;
//   train_small_kernel     the bias and head sums, split the same way;
//   train_reduce_kernel    adds the slabs in slab order and the rows' losses in row order.
// No float atomics anywhere: every number is a sum in a fixed order, so two calls on the same inputs give the same bits, and a row's
// probabilities do not depend on where in the batch it lies (the gates GEMM sums over k in an order that is the same for every chunk).
//
// Why the matrix-vector form of rec_small_kernel and not rec_kernel's 16 streams per workgroup: training batches are the reference's
// 128 rows, not the tens of thousands of an inference corpus.  16 rows a workgroup would occupy 8 of 256 CUs at B = 128; a row a
// workgroup occupies 128, and 1024 rows still fit as four workgroups a CU (256 VGPRs a thread, 2 waves a SIMD).
//
// Chunks behind n_chunks[b] are never read as numbers: the recurrences stop there, and the reductions replace both operands of such a
// chunk by zero (flags), whatever -- NaN included -- the feature tensor holds there.
#include <hip/hip_runtime.h>

#include "activations.hpp"
#include "device_api.hpp"
#include "trainer.hpp"

namespace vad {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int H = kTrainH, G = kTrainG, ST = kTrainStash;
constexpr uint8_t kLive = 1, kHasPrev = 2;

__device__ inline long clamp_chunks(long n, long T) { return n < 0 ? 0 : n > T ? T : n; }

// ---- GX = feat W_ih^T + b ------------------------------------------------------------------------------------------------------------
// MFMA operand maps (16x16x4): A[row l & 15][k l >> 4], B[k l >> 4][col l & 15], D[row 4 (l >> 4) + i][col l & 15].  The K index a lane
// supplies in MFMA number 4 m + s is 16 m + 4 (l >> 4) + s -- a permutation of 0 .. 127 that both operands share, so that each lane
// fetches its share as eight 16-byte loads.
__global__ void __launch_bounds__(256) train_gates_kernel(const float *feat, const float *w_ih, const float *b_ih, const float *b_hh, float *gx,
                                                          long N) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const long n0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (n0 >= N) return;
    const long row = n0 + r < N ? n0 + r : N - 1;             // (rows behind N: a copy of the last row, never stored)
    f32x4 a[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) a[m] = *reinterpret_cast<const f32x4 *>(feat + row * H + 16 * m + 4 * g);
#pragma unroll
    for (int ct = 0; ct < G / 16; ++ct) {
        const int col = 16 * ct + r;
        const float *wrow = w_ih + (size_t)col * H + 4 * g;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 8; m += 2) {
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(wrow + 16 * m);
            const f32x4 b1 = *reinterpret_cast<const f32x4 *>(wrow + 16 * (m + 1));
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], b0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m + 1][s], b1[s], acc1, 0, 0, 0);
            }
        }
        const float bias = b_ih[col] + b_hh[col];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long n = n0 + 4 * g + i;
            if (n < N) gx[n * G + col] = (acc0[i] + acc1[i]) + bias;
        }
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512) train_forward_kernel(const float *w_hh, const float *w_out, const float *b_out, const float *gx, long T,
                                                            const long *n_chunks, const uint8_t *labels, long ldl, const uint8_t *keep,
                                                            float keep_scale, float noise_loss, double denom, float *stash, float *dz,
                                                            uint8_t *flags, float *probs, double *row_loss) {
    __shared__ __attribute__((aligned(16))) float h_s[2][H];
    __shared__ float act_s[G];
    const int j = threadIdx.x, lane = j & 63;
    const long b = blockIdx.x, nc = clamp_chunks(n_chunks[b], T);
    for (long t = j; t < T; t += 512) {
        flags[b * T + t] = (uint8_t)((t < nc ? kLive : 0) | (t > 0 ? kHasPrev : 0));
        if (t >= nc) {
            dz[b * T + t] = 0.f;
            if (probs) probs[b * T + t] = 0.f;
        }
    }
    if (nc == 0) {
        if (j == 0) row_loss[b] = 0.0;
        return;
    }
    float w[H];
#pragma unroll
    for (int k = 0; k < H; k += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(w_hh + (size_t)j * H + k);
        w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
    }
    if (j < H) h_s[0][j] = 0.f;
    float c = 0.f;
    // the head's operands, wave 0: units lane and lane + 64
    const float wo0 = j < 64 ? w_out[lane] : 0.f, wo1 = j < 64 ? w_out[lane + 64] : 0.f, bo = b_out[0];
    double ls = 0.0;
    const bool is_g = j >= 2 * H && j < 3 * H;                // (whole waves: the gates are 128 rows each)
    float gx_next = gx[(b * T) * G + j];
    __syncthreads();
    for (long t = 0; t < nc; ++t) {
        const long n = b * T + t;
        const int cur = (int)(t & 1);
        const float gxv = gx_next;
        if (t + 1 < nc) gx_next = gx[(n + 1) * G + j];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const f32x4 hv = *reinterpret_cast<const f32x4 *>(&h_s[cur][k]);
            a0 = fmaf(w[k], hv[0], a0);
            a1 = fmaf(w[k + 1], hv[1], a1);
            a2 = fmaf(w[k + 2], hv[2], a2);
            a3 = fmaf(w[k + 3], hv[3], a3);
        }
        const float pre = gxv + ((a0 + a1) + (a2 + a3));
        const float act = is_g ? tanh_ulp_f(pre) : sigmoid_ulp_f(pre);
        act_s[j] = act;
        stash[n * ST + j] = act;
        __syncthreads();
        if (j < H) {
            const float i = act_s[j], f = act_s[H + j], gg = act_s[2 * H + j], o = act_s[3 * H + j];
            c = fmaf(f, c, i * gg);
            const float tc = tanh_ulp_f(c), h = o * tc;
            h_s[cur ^ 1][j] = h;
            stash[n * ST + G + j] = c;
            stash[n * ST + G + H + j] = tc;
            stash[n * ST + G + 2 * H + j] = h;
        }
        __syncthreads();
        if (j < 64) {                                          // the head of step t, while the other waves start step t + 1
            float y0 = relu_f(h_s[cur ^ 1][lane]), y1 = relu_f(h_s[cur ^ 1][lane + 64]);
            if (keep) {
                y0 = keep[n * H + lane] ? y0 * keep_scale : 0.f;
                y1 = keep[n * H + lane + 64] ? y1 * keep_scale : 0.f;
            }
            float s = fmaf(wo0, y0, wo1 * y1);
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            if (lane == 0) {
                const float p = sigmoid_ulp_f(s + bo);
                const unsigned lab = labels[b * ldl + t];
                const double wgt = train_weight(lab, (double)noise_loss);
                if (wgt != 0.0) ls += wgt * train_bce(p, lab);
                dz[n] = (float)train_dz(p, lab, wgt, denom);
                if (probs) probs[n] = p;
            }
        }
    }
    if (j == 0) row_loss[b] = ls;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512) train_backward_kernel(const float *w_hh, const float *w_out, long T, const long *n_chunks,
                                                             const uint8_t *keep, float keep_scale, const float *stash, const float *dz,
                                                             float *dg) {
    __shared__ __attribute__((aligned(16))) float dg_s[G];
    __shared__ float part_s[4][H];
    const int tid = threadIdx.x, q = tid >> 7, k = tid & (H - 1);
    const long b = blockIdx.x, nc = clamp_chunks(n_chunks[b], T);
    if (nc == 0) return;
    float w[H];
#pragma unroll
    for (int u = 0; u < H; ++u) w[u] = w_hh[(size_t)(q * H + u) * H + k];
    dg_s[tid] = 0.f;
    const float wo = w_out[k];
    float dc = 0.f;
    // what step t needs of the stash, fetched one step ahead (threads k < 128 only)
    float s_i = 0.f, s_f = 0.f, s_g = 0.f, s_o = 0.f, s_tc = 0.f, s_h = 0.f, s_cp = 0.f, s_dz = 0.f, s_kk = 1.f;
    auto fetch = [&](long t) {
        const long n = b * T + t;
        const float *s = stash + n * ST;
        s_i = s[k]; s_f = s[H + k]; s_g = s[2 * H + k]; s_o = s[3 * H + k];
        s_tc = s[G + H + k]; s_h = s[G + 2 * H + k];
        s_cp = t > 0 ? s[G + k - ST] : 0.f;
        s_dz = dz[n];
        s_kk = keep ? (keep[n * H + k] ? keep_scale : 0.f) : 1.f;
    };
    if (tid < H) fetch(nc - 1);
    __syncthreads();
    for (long t = nc - 1; t >= 0; --t) {
        const long n = b * T + t;
        const float i = s_i, f = s_f, gg = s_g, o = s_o, tc = s_tc, h = s_h, cp = s_cp, dzv = s_dz, kk = s_kk;
        if (tid < H && t > 0) fetch(t - 1);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int u = 0; u < H; u += 4) {
            const f32x4 dv = *reinterpret_cast<const f32x4 *>(&dg_s[q * H + u]);
            a0 = fmaf(w[u], dv[0], a0);
            a1 = fmaf(w[u + 1], dv[1], a1);
            a2 = fmaf(w[u + 2], dv[2], a2);
            a3 = fmaf(w[u + 3], dv[3], a3);
        }
        part_s[q][k] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (tid < H) {
            const float rec = (part_s[0][k] + part_s[1][k]) + (part_s[2][k] + part_s[3][k]);
            const float dh = (h > 0.f ? kk * wo * dzv : 0.f) + rec;
            const float d_o = dh * tc;
            const float d_c = fmaf(dh * o, 1.f - tc * tc, dc);
            const float gi = d_c * gg * i * (1.f - i), gf = d_c * cp * f * (1.f - f), g_g = d_c * i * (1.f - gg * gg), go = d_o * o * (1.f - o);
            dc = d_c * f;
            dg_s[k] = gi; dg_s[H + k] = gf; dg_s[2 * H + k] = g_g; dg_s[3 * H + k] = go;
            float *out = dg + n * G;
            out[k] = gi; out[H + k] = gf; out[2 * H + k] = g_g; out[3 * H + k] = go;
        }
        __syncthreads();
    }
}

// ---- dW = dG^T X over one split of N -----------------------------------------------------------------------------------------------------
// A wave owns 64 gate rows x 128 columns (32 accumulators); blockIdx.x = half of the gate rows, blockIdx.y = split, blockIdx.z = which
// product (0: X = feat, 1: X = h of the chunk before).  K runs over the split's chunks four at a time.
__global__ void __launch_bounds__(256) train_wgrad_kernel(const float *dg, const float *feat, const float *stash, const uint8_t *flags, long N,
                                                          long split_len, float *slabs) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    const bool prev = blockIdx.z == 1;
    const long s = blockIdx.y, k_begin = s * split_len, k_end = k_begin + split_len < N ? k_begin + split_len : N;
    f32x4 acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long kk = k_begin; kk < k_end; kk += 4) {
        const long n = kk + g;
        const uint8_t fl = n < k_end ? flags[n] : (uint8_t)0;
        const bool live = fl & kLive, use_x = live && (!prev || (fl & kHasPrev));
        float av[4], bv[8];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = live ? dg[n * G + j0 + 16 * a + r] : 0.f;
        const float *x = prev ? stash + (n - 1) * ST + G + 2 * H : feat + n * H;
#pragma unroll
        for (int c = 0; c < 8; ++c) bv[c] = use_x ? x[16 * c + r] : 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[c], acc[a][c], 0, 0, 0);
    }
    float *out = slabs + (size_t)s * kTrainSlabFloats + (prev ? (size_t)G * H : 0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[(size_t)(j0 + 16 * a + 4 * g + i) * H + 16 * c + r] = acc[a][c][i];
}

// the bias sums (thread j: gate row j), dw_out (threads < 128) and db_out (thread 128) of one split, each in chunk order
__global__ void __launch_bounds__(512) train_small_kernel(const float *dg, const float *stash, const float *dz, const uint8_t *flags,
                                                          const uint8_t *keep, float keep_scale, long N, long split_len, float *slabs) {
    const int j = threadIdx.x;
    const long s = blockIdx.x, k_begin = s * split_len, k_end = k_begin + split_len < N ? k_begin + split_len : N;
    float *out = slabs + (size_t)s * kTrainSlabFloats + 2 * (size_t)G * H;
    float sb = 0.f, sw = 0.f;
    for (long n = k_begin; n < k_end; ++n) {
        if (!(flags[n] & kLive)) continue;
        sb += dg[n * G + j];
        if (j < H) {
            float y = relu_f(stash[n * ST + G + 2 * H + j]);
            if (keep) y = keep[n * H + j] ? y * keep_scale : 0.f;
            sw = fmaf(dz[n], y, sw);
        } else if (j == H) {
            sw += dz[n];
        }
    }
    out[j] = sb;
    if (j <= H) out[G + j] = sw;
}

__global__ void __launch_bounds__(256) train_reduce_kernel(const float *slabs, long splits, const double *row_loss, int B, double denom, float *g_wih,
                                                           float *g_whh, float *g_bih, float *g_bhh, float *g_wout, float *g_bout, double *loss) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < kTrainSlabFloats) {
        float v = 0.f;
        for (long s = 0; s < splits; ++s) v += slabs[(size_t)s * kTrainSlabFloats + e];
        const size_t GH = (size_t)G * H;
        if (e < GH) g_wih[e] = v;
        else if (e < 2 * GH) g_whh[e - GH] = v;
        else if (e < 2 * GH + G) g_bih[e - 2 * GH] = g_bhh[e - 2 * GH] = v;
        else if (e < 2 * GH + G + H) g_wout[e - 2 * GH - G] = v;
        else g_bout[0] = v;
    }
    if (e == 0) {
        double t = 0.0;
        for (int b = 0; b < B; ++b) t += row_loss[b];
        *loss = t / denom;
    }
}

// ---- vad_encode_audio: gx (MFMA D-fragment order, kernels_ref.hip unpack_gx_kernel) -> feat[B][T][128], gate rows 0 .. 127 -------------
__global__ void unpack_feat_kernel(const float *gx, float *feat, int B, long T, long t0, long nt) {
    // feat[b][t0 + t][row] ; gx[st][t][mb][lane][r] with row = 16 mb + 4 g + r, b = 16 st + j
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)B * nt * H;
    if (idx >= total) return;
    const int row = (int)(idx % H);
    const long t = (idx / H) % nt;
    const long b = idx / (H * nt);
    const int mb = row >> 4, g = (row >> 2) & 3, r = row & 3, j = (int)(b & 15);
    const long st = b >> 4;
    feat[(b * T + t0 + t) * H + row] = gx[(((st * nt + t) * 32 + mb) * 64 + (g * 16 + j)) * 4 + r];
}

}  // namespace

hipError_t launch_unpack_feat(const float *gx, float *feat, int B, long T, long t0, long nt, hipStream_t s) {
    const long total = (long)B * nt * H;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_feat_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, gx, feat, B, T, t0, nt);
    return hipGetLastError();
}

hipError_t launch_decoder_grad(const TrainArgs &a, hipStream_t s) {
    const long N = (long)a.B * a.T;
    const TrainLayout l = train_layout(a.B, a.T);
    char *ws = static_cast<char *>(a.workspace);
    float *gx = reinterpret_cast<float *>(ws + l.gx), *dg = reinterpret_cast<float *>(ws + l.dg);
    float *stash = reinterpret_cast<float *>(ws + l.stash), *dz = reinterpret_cast<float *>(ws + l.dz);
    uint8_t *flags = reinterpret_cast<uint8_t *>(ws + l.flags);
    double *row_loss = reinterpret_cast<double *>(ws + l.row_loss);
    float *slabs = reinterpret_cast<float *>(ws + l.slabs);
    const long split_len = train_split_len(N), splits = train_splits(N);
    hipLaunchKernelGGL(train_gates_kernel, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, s, a.feat, a.w_ih, a.b_ih, a.b_hh, gx, N);
    hipLaunchKernelGGL(train_forward_kernel, dim3((unsigned)a.B), dim3(512), 0, s, a.w_hh, a.w_out, a.b_out, gx, a.T, a.n_chunks, a.labels, a.ldl,
                       a.keep, a.keep_scale, a.noise_loss, a.denom, stash, dz, flags, a.probs, row_loss);
    hipLaunchKernelGGL(train_backward_kernel, dim3((unsigned)a.B), dim3(512), 0, s, a.w_hh, a.w_out, a.T, a.n_chunks, a.keep, a.keep_scale, stash,
                       dz, dg);
    hipLaunchKernelGGL(train_wgrad_kernel, dim3(2, (unsigned)splits, 2), dim3(256), 0, s, dg, a.feat, stash, flags, N, split_len, slabs);
    hipLaunchKernelGGL(train_small_kernel, dim3((unsigned)splits), dim3(512), 0, s, dg, stash, dz, flags, a.keep, a.keep_scale, N, split_len, slabs);
    hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((kTrainSlabFloats + 255) / 256)), dim3(256), 0, s, slabs, splits, row_loss, a.B, a.denom,
                       a.g_wih, a.g_whh, a.g_bih, a.g_bhh, a.g_wout, a.g_bout, a.loss);
    return hipGetLastError();
}

}  // namespace vad
