// kernel_augment_x.hip -- the two augmentation ops of augment.hpp that cannot run in place, ALIAS and FIR, for
// vad_augment_rows_device_x, gfx950.  At op position p, a row that has one of them there is read from `out` and written to the
// scratch (the second row buffer); aug_x_copy_kernel then brings the row's len samples back and raises the row's non-finite flag if
// the op was the recipe's last.  Rows with another kind at that position, or nothing, leave all three kernels at once and are
// never copied.
//
// ALIAS  one thread per output sample: aug_alias_sample of the header, in double, the statements the twin runs; bit-equal.
//
// FIR    y[n] = sum_k h[k] x[n - k] in direct form on v_mfma_f32_16x16x4_f32, as a Hankel product.  A wave owns 256 consecutive
//   outputs per accumulator, y[b_j + m] with b_j = n0 + 16 j:  y[b_j + m] = sum over d of A[m][d] B[d][j],  A[m][d] = h[d + m] (zero
//   outside [0, K)),  B[d][j] = x[b_j - d] (zero before the row's start), d = -15 .. K - 1: every multiply-add of the instruction
//   is one of the sum's (but for the 15 + 15 d at the two ends), so 256 outputs cost (K + 15) / 4 instructions, rounded up to 4.
//   The fp32 MFMA is a chain of fused multiply-adds in ascending d, which for one output is ascending k: the order of a sample's
//   sum depends on (K, n) alone, and the zero entries add exactly nothing.
//   A workgroup of four waves owns 4096 outputs, a wave 1024 in four accumulators that share the A operand.  The taps go through
//   LDS in slices of 512 d; with a slice goes the window of 4592 samples it meets, stored as four planes by (index mod 4): a lane's
//   B operand steps down four samples per instruction, so one 16-byte read of its plane feeds four instructions (16 lanes read
//   256 contiguous bytes: no bank conflict), and its A operand is four 4-byte reads in which the 64 lanes touch 19 consecutive
//   words.  Per sixteen instructions a wave issues four 16-byte and four 4-byte LDS reads.
//   Taps behind the bank's K are staged as zeros, never read; taps no output of the workgroup reaches (k > n) are not visited.
//   An output that is not finite (an infinite sample, or one met by a zero of A) is computed again by its lane as the plain chain
//   over its own K taps, so that a row's non-finite samples are the rule's and no others.
// No atomics; every value is produced by one lane in a fixed order.
#include <hip/hip_runtime.h>

#include "augment.hpp"
#include "device_api.hpp"

namespace vad {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFirThreads = 256;
constexpr int kFirTiles = 4;                                   // accumulators (256 outputs each) of one wave
constexpr int kFirWaveOut = 256 * kFirTiles;
constexpr int kFirOut = kFirWaveOut * (kFirThreads / 64);      // outputs of one workgroup
constexpr int kFirSlice = 512;                                 // d of one staged slice
constexpr int kFirGroups = kFirSlice / 16;                     // groups of four instructions per slice
constexpr int kFirWin = kFirOut - 16 + kFirSlice;              // samples a slice meets
constexpr int kFirPlane = kFirWin / 4;
constexpr int kFirTaps = kFirSlice + 16;
static_assert(kFirWin % 16 == 0 && kFirPlane % 4 == 0, "planes are read 16 bytes at a time");

struct XWs {
    const long *len;
    const int *n_ops;
    int *flag;
};
inline XWs x_ws(void *workspace, long n, long width) {
    const AugLayout l = aug_layout(n, width);
    char *w = static_cast<char *>(workspace);
    return XWs{reinterpret_cast<const long *>(w + l.len), reinterpret_cast<const int *>(w + l.n_ops), reinterpret_cast<int *>(w + l.flag)};
}

__device__ inline bool finite_f(float v) { return v - v == 0.0f; }

// the op of this row at this position, or nullptr
__device__ inline const vad_augment_op *op_at(const vad_augment_recipe *recipes, const XWs &ws, long row, int pos, bool *last) {
    const int n_ops = ws.n_ops[row];
    if (pos >= n_ops) return nullptr;
    *last = pos == n_ops - 1;
    return &recipes[row].ops[pos];
}

__global__ void __launch_bounds__(256) aug_alias_kernel(const vad_augment_recipe *recipes, int pos, const float *out, float *scratch, long ld_out, XWs ws) {
    const long row = blockIdx.y;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, &last);
    if (!op || op->kind != VAD_AUGMENT_ALIAS) return;
    const long len = ws.len[row];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const float *x = out + (size_t)row * ld_out;
    const long m = aug_alias_m(len, op->a, op->b);
    scratch[(size_t)row * ld_out + i] = m == 0 ? x[i] : aug_alias_sample(aug_alias_plan(len, m), x, i);
}

__global__ void __launch_bounds__(kFirThreads) aug_fir_kernel(const vad_augment_recipe *recipes, int pos, const float *bank, const float *out,
                                                               float *scratch, long ld_out, XWs ws) {
    __shared__ __attribute__((aligned(16))) float xs[4][kFirPlane];
    __shared__ float hs[kFirTaps];
    const long row = blockIdx.y;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, &last);
    if (!op || op->kind != VAD_AUGMENT_FIR) return;
    const long len = ws.len[row], n0 = (long)blockIdx.x * kFirOut;
    if (n0 >= len) return;
    const int K = op->n_sections;
    const float *h = bank + op->seed;
    const float *x = out + (size_t)row * ld_out;
    const long reach = n0 + kFirOut < len ? n0 + kFirOut : len;              // taps k >= reach meet no sample of these outputs
    const int Keff = (long)K < reach ? K : (int)reach;
    const int D = Keff + 15;                                                 // d = -15 .. Keff - 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;                                // A: m = lo, k = hi;  B: j = lo, k = hi
    const bool busy = n0 + (long)wave * kFirWaveOut < len;
    f32x4 acc[kFirTiles];
#pragma unroll
    for (int t = 0; t < kFirTiles; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c * kFirSlice < D; ++c) {
        __syncthreads();
        for (int i = tid; i < kFirTaps; i += kFirThreads) {                  // hs[i] = h[512 c - 15 + i]
            const int t = c * kFirSlice - 15 + i;
            hs[i] = (t >= 0 && t < Keff) ? h[t] : 0.0f;
        }
        const long p0 = n0 - (long)c * kFirSlice - (kFirSlice - 16);         // the window's first sample, a multiple of 16
        for (int i = tid; i < kFirPlane; i += kFirThreads) {
            const long p = p0 + 4 * (long)i;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (p >= 0 && p < ld_out) v = *reinterpret_cast<const float4 *>(x + p);
            xs[0][i] = v.x;
            xs[1][i] = v.y;
            xs[2][i] = v.z;
            xs[3][i] = v.w;
        }
        __syncthreads();
        if (!busy) continue;
        const int left = (D - c * kFirSlice + 15) / 16, groups = left < kFirGroups ? left : kFirGroups;
        const float *ap = hs + lo + hi;
        const float *bp = &xs[3 - hi][wave * (kFirWaveOut / 4) + kFirSlice / 4 + 4 * lo - 4];
        for (int g = 0; g < groups; ++g) {
            float a[4];
            f32x4 b[kFirTiles];
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = ap[16 * g + 4 * s];
#pragma unroll
            for (int t = 0; t < kFirTiles; ++t) b[t] = *reinterpret_cast<const f32x4 *>(bp + 64 * t - 4 * g);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < kFirTiles; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[t][3 - s], acc[t], 0, 0, 0);
        }
    }
    if (!busy) return;
    float *y = scratch + (size_t)row * ld_out;
#pragma unroll
    for (int t = 0; t < kFirTiles; ++t) {
        const long at = n0 + (long)wave * kFirWaveOut + 256 * t + 16 * lo + 4 * hi;      // C: column lo, rows 4 hi .. 4 hi + 3
        if (at >= len) continue;
        float v[4] = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (!finite_f(v[r]) && at + r < len) {
                const long n = at + r, top = n < K - 1 ? n : K - 1;
                float sum = 0.0f;
                for (long k = 0; k <= top; ++k) sum = fmaf(h[k], x[n - k], sum);
                v[r] = sum;
            }
        *reinterpret_cast<float4 *>(y + at) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// out[row][0 .. len) <- scratch, in the rows that have ALIAS or FIR at this position
__global__ void __launch_bounds__(256) aug_x_copy_kernel(const vad_augment_recipe *recipes, int pos, const float *scratch, float *out, long ld_out, XWs ws) {
    const long row = blockIdx.y;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, &last);
    if (!op || (op->kind != VAD_AUGMENT_ALIAS && op->kind != VAD_AUGMENT_FIR)) return;
    const long len = ws.len[row];
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= len) return;
    const float4 q = *reinterpret_cast<const float4 *>(scratch + (size_t)row * ld_out + i);
    float v[4] = {q.x, q.y, q.z, q.w};
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i + k >= len) v[k] = 0.0f;
        bad |= !finite_f(v[k]);
    }
    *reinterpret_cast<float4 *>(out + (size_t)row * ld_out + i) = make_float4(v[0], v[1], v[2], v[3]);
    if (last && bad) ws.flag[row] = 1;
}

}  // namespace

hipError_t launch_augment_x(const AugArgs &a, int pos, hipStream_t s) {
    const XWs ws = x_ws(a.workspace, a.n, a.ld_out);
    const unsigned rows = (unsigned)a.n;
    hipLaunchKernelGGL(aug_alias_kernel, dim3((unsigned)((a.ld_out + 255) / 256), rows), dim3(256), 0, s, a.recipes, pos, a.out, a.scratch, a.ld_out, ws);
    hipLaunchKernelGGL(aug_fir_kernel, dim3((unsigned)((a.ld_out + kFirOut - 1) / kFirOut), rows), dim3(kFirThreads), 0, s, a.recipes, pos, a.bank,
                       a.out, a.scratch, a.ld_out, ws);
    hipLaunchKernelGGL(aug_x_copy_kernel, dim3((unsigned)((a.ld_out + 1023) / 1024), rows), dim3(256), 0, s, a.recipes, pos, a.scratch, a.out, a.ld_out, ws);
    return hipGetLastError();
}

}  // namespace vad
