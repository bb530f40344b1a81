// kernel_augment.hip -- the augmentation ops of augment.hpp on a padded batch (vad_augment_rows_device), gfx950.
//
// The batch is converted to float32 in `out` once (zero behind len); every op then works on `out` in place, one op position after the
// other.  A kernel of position p leaves at once in a row whose recipe has another kind there, or nothing.
//
// NOISE   one thread per four samples: one Philox block, one 16-byte load and store.
// BIQUADS a time recursion; 128 rows are two waves, so a row is cut into blocks of kAugBlock samples and a lane owns a block:
//   (i)   biquad_state_kernel: every block but the row's last runs the cascade from zero state and keeps the final state (2 S doubles);
//   (ii)  biquad_scan_kernel: one wave per row builds M, the zero-input transition of one block (the cascade driven from the 2 S unit
//         states, one lane each), and walks the blocks in order, s[b + 1] = M s[b] + z[b], leaving the INCOMING state of every block;
//   (iii) biquad_apply_kernel: every block runs the cascade again from its incoming state and writes float32.
//   A wave owns 64 consecutive blocks.  A lane walks its block while its neighbours walk theirs, a stride of one block apart: the
//   samples go through an LDS tile of 64 blocks x 32 samples, loaded and stored as 16-byte accesses in which 8 lanes cover 128
//   contiguous bytes of one block; rows of the tile are 33 words apart, so both the 64 lanes reading a column and the lanes filling
//   it touch 32 different banks.  The recursion is in double; S is rounded up to 1, 2, 4 or 8 with identity sections (b0 = 1), which
//   pass a value and a zero state through exactly, so that coefficients and states are registers.
// CLIP    one workgroup per row: a radix select over the order-preserving keys, four 8-bit digits from the top, for the (at most)
//   four order statistics the two quantiles interpolate between -- targets that still share their leading digits share a histogram
//   -- with integer LDS counters; then the clip over the row.
// ALIAS, FIR (vad_augment_rows_device_x only): kernel_augment_x.hip, through a second row buffer.
// No float atomics anywhere; every value is produced by one thread in a fixed order.
#include <hip/hip_runtime.h>

#include "augment.hpp"
#include "device_api.hpp"

namespace vad {
namespace {

constexpr int kTile = 32;                          // samples of a block in one LDS tile
constexpr int kLanes = 64;                         // blocks of one wave
constexpr int kClipThreads = 1024;

struct AugWs {
    long *len;
    int *n_ops;
    int *flag;
    double *state;
    long nb;
};
inline AugWs aug_ws(void *workspace, long n, long width) {
    const AugLayout l = aug_layout(n, width);
    char *w = static_cast<char *>(workspace);
    return AugWs{reinterpret_cast<long *>(w + l.len), reinterpret_cast<int *>(w + l.n_ops), reinterpret_cast<int *>(w + l.flag),
                 reinterpret_cast<double *>(w + l.state), l.nb};
}

__device__ inline bool finite_f(float v) { return v - v == 0.0f; }

__global__ void __launch_bounds__(256) aug_plan_kernel(const long *lens, const vad_augment_recipe *recipes, long n, long max_len, long bank_len, AugWs ws) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long l = lens[i];
    ws.len[i] = l < 0 ? 0 : (l > max_len ? max_len : l);
    ws.n_ops[i] = aug_check(recipes[i], bank_len) == 0 ? recipes[i].n_ops : 0;
    ws.flag[i] = 0;
}

// out[row][0 .. ld_out) = float32 of the input, zero behind len.  kRestore: only the rows whose flag is set.
template <typename T, bool kRestore>
__global__ void __launch_bounds__(256) aug_convert_kernel(const T *pcm, long ld, float *out, long ld_out, AugWs ws) {
    const long row = blockIdx.y;
    if (kRestore && !ws.flag[row]) return;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= ld_out) return;
    const long len = ws.len[row];
    const T *x = pcm + (size_t)row * ld;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = 0.0f;
        if (i + k < len) v[k] = sizeof(T) == 2 ? (float)x[i + k] / 32768.0f : (float)x[i + k];
    }
    *reinterpret_cast<float4 *>(out + (size_t)row * ld_out + i) = make_float4(v[0], v[1], v[2], v[3]);
}

// the op of this row at this position if it is of `kind`, else nullptr
__device__ inline const vad_augment_op *op_at(const vad_augment_recipe *recipes, const AugWs &ws, long row, int pos, int kind, bool *last) {
    const int n_ops = ws.n_ops[row];
    if (pos >= n_ops) return nullptr;
    const vad_augment_op *op = &recipes[row].ops[pos];
    *last = pos == n_ops - 1;
    return op->kind == kind ? op : nullptr;
}

__global__ void __launch_bounds__(256) aug_noise_kernel(const vad_augment_recipe *recipes, int pos, float *out, long ld_out, AugWs ws) {
    const long row = blockIdx.y;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, VAD_AUGMENT_NOISE, &last);
    if (!op) return;
    const long len = ws.len[row];
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= len) return;
    float g[4];
    aug_gauss4(op->seed, recipes[row].row_key, (uint64_t)(i >> 2), g);
    const float amp = (float)op->a;
    float4 *p = reinterpret_cast<float4 *>(out + (size_t)row * ld_out + i);
    const float4 x = *p;
    float v[4] = {x.x, x.y, x.z, x.w};
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i + k < len) {
            v[k] = aug_add_noise(v[k], amp, g[k]);
            bad |= !finite_f(v[k]);
        }
    *p = make_float4(v[0], v[1], v[2], v[3]);
    if (last && bad) ws.flag[row] = 1;
}

// ---- BIQUADS ---------------------------------------------------------------------------------------------------------------------
template <int NS>
__device__ inline void load_coef(const vad_augment_op *op, double (*c)[5]) {
    const int ns = op->n_sections;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int k = 0; k < 5; ++k) c[s][k] = s < ns ? op->coef[s][k] : (k == 0 ? 1.0 : 0.0);
}

// the tile <- 32 samples from i0 of the 64 blocks from blk0 (zero behind ld_out); the lanes of a wave together
__device__ inline void tile_load(float (*tile)[kTile + 1], const float *row, long blk0, int i0, long ld_out, int lane) {
#pragma unroll
    for (int it = 0; it < kLanes / 8; ++it) {
        const int blk = it * 8 + (lane >> 3), off = (lane & 7) * 4;
        const long i = (blk0 + blk) * (long)kAugBlock + i0 + off;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < ld_out) v = *reinterpret_cast<const float4 *>(row + i);
        tile[blk][off] = v.x;
        tile[blk][off + 1] = v.y;
        tile[blk][off + 2] = v.z;
        tile[blk][off + 3] = v.w;
    }
}
__device__ inline void tile_store(const float (*tile)[kTile + 1], float *row, long blk0, int i0, long ld_out, long n_blocks, int lane) {
#pragma unroll
    for (int it = 0; it < kLanes / 8; ++it) {
        const int blk = it * 8 + (lane >> 3), off = (lane & 7) * 4;
        const long i = (blk0 + blk) * (long)kAugBlock + i0 + off;
        if (blk0 + blk < n_blocks && i < ld_out)
            *reinterpret_cast<float4 *>(row + i) = make_float4(tile[blk][off], tile[blk][off + 1], tile[blk][off + 2], tile[blk][off + 3]);
    }
}

template <int NS>
__device__ inline void state_pass(const vad_augment_op *op, const float *row, long blk0, long n_blocks, long ld_out, double *state_row,
                                  float (*tile)[kTile + 1]) {
    const int lane = threadIdx.x;
    double c[NS][5], st[2 * NS];
    load_coef<NS>(op, c);
#pragma unroll
    for (int s = 0; s < 2 * NS; ++s) st[s] = 0.0;
    const bool mine = blk0 + lane < n_blocks - 1;
    for (int i0 = 0; i0 < kAugBlock; i0 += kTile) {
        __syncthreads();
        tile_load(tile, row, blk0, i0, ld_out, lane);
        __syncthreads();
        if (mine)
            for (int k = 0; k < kTile; ++k) aug_cascade_step<NS>(c, st, (double)tile[lane][k]);
    }
    if (mine) {
        double *z = state_row + (blk0 + lane) * kAugStates;
#pragma unroll
        for (int s = 0; s < 2 * NS; ++s) z[s] = st[s];
    }
}

template <int NS>
__device__ inline void apply_pass(const vad_augment_op *op, float *row, long blk0, long n_blocks, long len, long ld_out, const double *state_row,
                                  float (*tile)[kTile + 1], bool last, int *flag) {
    const int lane = threadIdx.x;
    double c[NS][5], st[2 * NS];
    load_coef<NS>(op, c);
    const bool mine = blk0 + lane < n_blocks;
#pragma unroll
    for (int s = 0; s < 2 * NS; ++s) st[s] = mine ? state_row[(blk0 + lane) * kAugStates + s] : 0.0;
    bool bad = false;
    for (int i0 = 0; i0 < kAugBlock; i0 += kTile) {
        __syncthreads();
        tile_load(tile, row, blk0, i0, ld_out, lane);
        __syncthreads();
        if (mine) {
            const long at = (blk0 + lane) * (long)kAugBlock + i0;
            for (int k = 0; k < kTile; ++k) {
                float y = (float)aug_cascade_step<NS>(c, st, (double)tile[lane][k]);
                if (at + k >= len) y = 0.0f;
                bad |= !finite_f(y);
                tile[lane][k] = y;
            }
        }
        __syncthreads();
        tile_store(tile, row, blk0, i0, ld_out, n_blocks, lane);
    }
    if (last && bad) *flag = 1;
}

__global__ void __launch_bounds__(kLanes) biquad_state_kernel(const vad_augment_recipe *recipes, int pos, const float *out, long ld_out, AugWs ws) {
    __shared__ float tile[kLanes][kTile + 1];
    const long row = blockIdx.y;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, VAD_AUGMENT_BIQUADS, &last);
    if (!op) return;
    const long len = ws.len[row], n_blocks = (len + kAugBlock - 1) / kAugBlock, blk0 = (long)blockIdx.x * kLanes;
    if (blk0 >= n_blocks - 1) return;                          // (the last block's final state is nobody's input)
    const float *x = out + (size_t)row * ld_out;
    double *state_row = ws.state + (size_t)row * ws.nb * kAugStates;
    const int ns = op->n_sections;
    if (ns <= 1) state_pass<1>(op, x, blk0, n_blocks, ld_out, state_row, tile);
    else if (ns == 2) state_pass<2>(op, x, blk0, n_blocks, ld_out, state_row, tile);
    else if (ns <= 4) state_pass<4>(op, x, blk0, n_blocks, ld_out, state_row, tile);
    else state_pass<8>(op, x, blk0, n_blocks, ld_out, state_row, tile);
}

template <int NS>
__device__ inline void scan_pass(const vad_augment_op *op, long n_blocks, double *state_row, double (*Ms)[kAugStates + 1], double (*sv)[kAugStates]) {
    constexpr int D = 2 * NS;
    const int lane = threadIdx.x;
    double c[NS][5], st[D];
    load_coef<NS>(op, c);
    if (lane < D) {                                            // column `lane` of M: the block's zero-input response to unit state `lane`
#pragma unroll
        for (int s = 0; s < D; ++s) st[s] = s == lane ? 1.0 : 0.0;
        for (int k = 0; k < kAugBlock; ++k) aug_cascade_step<NS>(c, st, 0.0);
#pragma unroll
        for (int s = 0; s < D; ++s) Ms[s][lane] = st[s];
    }
    __syncthreads();
    double m[D];
#pragma unroll
    for (int j = 0; j < D; ++j) m[j] = lane < D ? Ms[lane][j] : 0.0;
    double s = 0.0;                                            // component `lane` of the state coming into block b
    for (long b0 = 0; b0 < n_blocks; b0 += 8) {
        double z[8];                                           // eight blocks' final states requested together, ahead of the walk
#pragma unroll
        for (int u = 0; u < 8; ++u) z[u] = (lane < D && b0 + u < n_blocks - 1) ? state_row[(b0 + u) * kAugStates + lane] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (b0 + u < n_blocks) {                           // (uniform over the wave)
                if (lane < D) {
                    state_row[(b0 + u) * kAugStates + lane] = s;
                    sv[u & 1][lane] = s;
                }
                __syncthreads();
                double acc = z[u];
#pragma unroll
                for (int j = 0; j < D; ++j) acc += m[j] * sv[u & 1][j];
                s = acc;
            }
        }
    }
}

__global__ void __launch_bounds__(kLanes) biquad_scan_kernel(const vad_augment_recipe *recipes, int pos, AugWs ws) {
    __shared__ double Ms[kAugStates][kAugStates + 1];
    __shared__ double sv[2][kAugStates];
    const long row = blockIdx.x;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, VAD_AUGMENT_BIQUADS, &last);
    if (!op) return;
    const long len = ws.len[row], n_blocks = (len + kAugBlock - 1) / kAugBlock;
    if (n_blocks == 0) return;
    double *state_row = ws.state + (size_t)row * ws.nb * kAugStates;
    const int ns = op->n_sections;
    if (ns <= 1) scan_pass<1>(op, n_blocks, state_row, Ms, sv);
    else if (ns == 2) scan_pass<2>(op, n_blocks, state_row, Ms, sv);
    else if (ns <= 4) scan_pass<4>(op, n_blocks, state_row, Ms, sv);
    else scan_pass<8>(op, n_blocks, state_row, Ms, sv);
}

__global__ void __launch_bounds__(kLanes) biquad_apply_kernel(const vad_augment_recipe *recipes, int pos, float *out, long ld_out, AugWs ws) {
    __shared__ float tile[kLanes][kTile + 1];
    const long row = blockIdx.y;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, VAD_AUGMENT_BIQUADS, &last);
    if (!op) return;
    const long len = ws.len[row], n_blocks = (len + kAugBlock - 1) / kAugBlock, blk0 = (long)blockIdx.x * kLanes;
    if (blk0 >= n_blocks) return;
    float *x = out + (size_t)row * ld_out;
    const double *state_row = ws.state + (size_t)row * ws.nb * kAugStates;
    const int ns = op->n_sections;
    if (ns <= 1) apply_pass<1>(op, x, blk0, n_blocks, len, ld_out, state_row, tile, last, ws.flag + row);
    else if (ns == 2) apply_pass<2>(op, x, blk0, n_blocks, len, ld_out, state_row, tile, last, ws.flag + row);
    else if (ns <= 4) apply_pass<4>(op, x, blk0, n_blocks, len, ld_out, state_row, tile, last, ws.flag + row);
    else apply_pass<8>(op, x, blk0, n_blocks, len, ld_out, state_row, tile, last, ws.flag + row);
}

// ---- CLIP ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kClipThreads) aug_clip_kernel(const vad_augment_recipe *recipes, int pos, float *out, long ld_out, AugWs ws) {
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t prefix[4];                             // the leading digits of target t found so far
    __shared__ long rank[4];                                   // its rank among the keys that share them
    __shared__ int owner[4];                                   // the first target with the same leading digits: its histogram counts
    __shared__ double gamma[2];
    __shared__ float lohi[2];
    const long row = blockIdx.x;
    bool last = false;
    const vad_augment_op *op = op_at(recipes, ws, row, pos, VAD_AUGMENT_CLIP, &last);
    if (!op) return;
    const long len = ws.len[row];
    if (len == 0) return;
    const int tid = threadIdx.x;
    float *x = out + (size_t)row * ld_out;
    const uint32_t *xb = reinterpret_cast<const uint32_t *>(x);
    if (tid == 0) {
        long p, n;
        aug_quantile_pos(len, op->a, &p, &n, &gamma[0]);
        rank[0] = p;
        rank[1] = n;
        aug_quantile_pos(len, op->b, &p, &n, &gamma[1]);
        rank[2] = p;
        rank[3] = n;
        for (int t = 0; t < 4; ++t) {
            prefix[t] = 0u;
            owner[t] = 0;
        }
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid >> 8][tid & 255] = 0u;
        __syncthreads();
        uint32_t pre[4];
        bool own[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pre[t] = prefix[t];
            own[t] = owner[t] == t;
        }
        for (long i = tid; i < len; i += kClipThreads) {
            const uint32_t key = aug_key(xb[i]);
            const uint32_t lead = shift == 24 ? 0u : key >> (shift + 8), digit = (key >> shift) & 255u;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (own[t] && lead == pre[t]) atomicAdd(&hist[t][digit], 1u);
        }
        __syncthreads();
        if (tid < 4) {
            const uint32_t *h = hist[owner[tid]];
            long r = rank[tid], below = 0;
            int d = 0;
            for (; d < 255; ++d) {
                const long cnt = (long)h[d];
                if (r < below + cnt) break;
                below += cnt;
            }
            prefix[tid] = (prefix[tid] << 8) | (uint32_t)d;
            rank[tid] = r - below;
        }
        __syncthreads();
        if (tid == 0)
            for (int t = 1; t < 4; ++t) {
                int o = t;
                for (int u = t - 1; u >= 0; --u)
                    if (prefix[u] == prefix[t]) o = u;
                owner[t] = o;
            }
        __syncthreads();
    }
    if (tid == 0) {
        lohi[0] = aug_lerp(__uint_as_float(aug_unkey(prefix[0])), __uint_as_float(aug_unkey(prefix[1])), gamma[0]);
        lohi[1] = aug_lerp(__uint_as_float(aug_unkey(prefix[2])), __uint_as_float(aug_unkey(prefix[3])), gamma[1]);
    }
    __syncthreads();
    const float lo = lohi[0], hi = lohi[1];
    bool bad = false;
    for (long i = (long)tid * 4; i < len; i += (long)kClipThreads * 4) {
        float4 *p = reinterpret_cast<float4 *>(x + i);
        const float4 q = *p;
        float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < len) {
                v[k] = aug_clip(v[k], lo, hi);
                bad |= !finite_f(v[k]);
            }
        *p = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (last && bad) ws.flag[row] = 1;
}

template <typename T>
void launch_convert(const AugArgs &a, const AugWs &ws, bool restore, hipStream_t s) {
    const dim3 grid((unsigned)((a.ld_out + 1023) / 1024), (unsigned)a.n);
    const T *pcm = static_cast<const T *>(a.pcm);
    if (restore) hipLaunchKernelGGL((aug_convert_kernel<T, true>), grid, dim3(256), 0, s, pcm, a.ld, a.out, a.ld_out, ws);
    else hipLaunchKernelGGL((aug_convert_kernel<T, false>), grid, dim3(256), 0, s, pcm, a.ld, a.out, a.ld_out, ws);
}

}  // namespace

hipError_t launch_augment(const AugArgs &a, hipStream_t s) {
    const AugWs ws = aug_ws(a.workspace, a.n, a.ld_out);
    const long max_len = a.ld < a.ld_out ? a.ld : a.ld_out;
    hipLaunchKernelGGL(aug_plan_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.lens, a.recipes, a.n, max_len, a.bank_len, ws);
    if (a.elem_size == 2) launch_convert<int16_t>(a, ws, false, s);
    else launch_convert<float>(a, ws, false, s);
    const dim3 elementwise((unsigned)((a.ld_out + 1023) / 1024), (unsigned)a.n);
    const dim3 groups((unsigned)((ws.nb + kLanes - 1) / kLanes), (unsigned)a.n);
    for (int pos = 0; pos < kAugMaxOps; ++pos) {
        hipLaunchKernelGGL(aug_noise_kernel, elementwise, dim3(256), 0, s, a.recipes, pos, a.out, a.ld_out, ws);
        hipLaunchKernelGGL(biquad_state_kernel, groups, dim3(kLanes), 0, s, a.recipes, pos, a.out, a.ld_out, ws);
        hipLaunchKernelGGL(biquad_scan_kernel, dim3((unsigned)a.n), dim3(kLanes), 0, s, a.recipes, pos, ws);
        hipLaunchKernelGGL(biquad_apply_kernel, groups, dim3(kLanes), 0, s, a.recipes, pos, a.out, a.ld_out, ws);
        hipLaunchKernelGGL(aug_clip_kernel, dim3((unsigned)a.n), dim3(kClipThreads), 0, s, a.recipes, pos, a.out, a.ld_out, ws);
        if (a.bank_len >= 0) (void)launch_augment_x(a, pos, s);
    }
    if (a.elem_size == 2) launch_convert<int16_t>(a, ws, true, s);
    else launch_convert<float>(a, ws, true, s);
    return hipGetLastError();
}

}  // namespace vad
