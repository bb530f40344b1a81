// kernel_collect.hip -- the speech (or the non-speech) of every row of a batch, packed: collect_chunks / drop_chunks (reference
// src/silero_vad/utils_vad.py:552-655) for all recordings of a bucket at once, on the batch that the ingest left in HBM.
//
// After the scan (kernel_scan.hip) a bucket's rows and its segment lists sit side by side in device memory.  What the caller of a VAD
// wants next is the audio inside (or outside) those segments; this kernel copies exactly those samples of every row into one packed
// buffer, so that only the kept bytes leave the device -- or none, for a consumer on the same GPU.  The parts of a row and what they
// keep are collector.hpp, the same source the host twin (vad_collect_segments) compiles.
//
//   * COUNT (count_kept_kernel, one lane per row): kept[i] = samples row i keeps; -1 for a row whose segment list did not fit its cap
//     (the list is incomplete: such a row is the host's).  The host turns kept[] into out_offset[] (an exclusive sum of the kept
//     counts, each rounded up to 16 bytes) between the two launches.
//   * GATHER (collect_segments_kernel): work is dealt by OUTPUT tile.  A persistent grid of one-wave workgroups walks the
//     (row, 8 KiB output tile) pairs; a tile behind the row's last kept sample is left at once.  Per item the wave builds the prefix
//     of the row's part lengths (a wave scan, 64 parts at a time) and keeps it in LDS beside the parts' first samples; a lane owns
//     16 output bytes, 8 times per tile, and finds its part by a binary search of that prefix.
//       fast path  the lane's 16 bytes lie inside one part of a batch at the 16 kHz rate (step 1): the source starts at ANY element,
//                  so the lane reads the aligned 16-byte granule that holds its first byte and, where that byte is not the granule's
//                  first, the next one -- a granule that holds a wanted byte lies in the row -- and funnels the 16 wanted bytes out
//                  of the pair (v_alignbyte, as the misaligned rows of kernel_ingest.hip); one aligned 16-byte store.  The 8 vectors'
//                  loads are issued before the first store.
//       slow path  a lane whose 16 bytes straddle parts, every lane of a raw-rate batch (step 2, 3: every step-th element), a row's
//                  last partial vector, a row whose destination is not 16-byte aligned: element by element.
//     Exactly kept[i] elements are written per row; the padding between rows is never touched.
//   * sources and destination are HBM: the wide grid of the device-source ingest kernels, not the 96 waves sized for PCIe.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "collector.hpp"
#include "device_api.hpp"

namespace vad {
namespace {

constexpr int kTileBytes = 8192;                   // one wave-iteration: 64 lanes x 16 B x 8
constexpr int kMaxParts = kCollectMaxCap + 1;      // (invert: one more part than segments)
using u32x4 = unsigned __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64) count_kept_kernel(long ld, int step, long n_rows, const long *audio_len, const vad_segment *segs,
                                                        long cap, const long *counts, int invert, long *kept) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    long n = counts[i];
    if (n > cap) {
        kept[i] = -1;
        return;
    }
    n = n < 0 ? 0 : n;
    const int64_t len = row_samples(audio_len[i], ld, step);
    const long parts = collect_parts(n, invert);
    long sum = 0;
    for (long k = 0; k < parts; ++k) {
        const Part p = collect_part(segs + i * cap, n, k, len, invert);
        sum += p.b > p.a ? (long)(p.b - p.a) : 0;
    }
    kept[i] = sum;
}

// bytes [m, m + 16) of the 32 bytes c ++ n; m differs from lane to lane
__device__ __forceinline__ u32x4 funnel(u32x4 c, u32x4 n, int m) {
    const int dq = m >> 2;
    const unsigned w0 = dq == 0 ? c.x : dq == 1 ? c.y : dq == 2 ? c.z : c.w;
    const unsigned w1 = dq == 0 ? c.y : dq == 1 ? c.z : dq == 2 ? c.w : n.x;
    const unsigned w2 = dq == 0 ? c.z : dq == 1 ? c.w : dq == 2 ? n.x : n.y;
    const unsigned w3 = dq == 0 ? c.w : dq == 1 ? n.x : dq == 2 ? n.y : n.z;
    const unsigned w4 = dq == 0 ? n.x : dq == 1 ? n.y : dq == 2 ? n.z : n.w;
    const unsigned r = (unsigned)m & 3u;                       // v_alignbyte_b32: ({hi, lo} >> 8 r) & 0xffffffff
    return u32x4{__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r), __builtin_amdgcn_alignbyte(w3, w2, r),
                 __builtin_amdgcn_alignbyte(w4, w3, r)};
}

template <int ESZ>
__global__ void __launch_bounds__(64) collect_segments_kernel(const uint8_t *pcm, long ld, int step, long n_rows, const long *audio_len,
                                                              const vad_segment *segs, long cap, const long *counts, int invert,
                                                              const long *kept, const long *out_offset, uint8_t *out,
                                                              long tiles_per_row) {
    constexpr int EPV = 16 / ESZ;                  // elements of a lane's vector
    constexpr long EPT = kTileBytes / ESZ;         // elements of a tile
    using elem_t = typename std::conditional<ESZ == 2, unsigned short, unsigned>::type;
    __shared__ long long s_incl[kMaxParts];        // output elements of the row up to and including part k
    __shared__ long long s_first[kMaxParts];       // part k's first sample
    const int lane = threadIdx.x;
    const long items = n_rows * tiles_per_row;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        // everything up to the vectors is wave-uniform
        const long row = item / tiles_per_row, tile0 = item % tiles_per_row;
        const long want = kept[row];
        long n = counts[row];
        if (want <= 0 || tile0 * EPT >= want || n > cap) continue;
        n = n < 0 ? 0 : n;
        const int64_t len = row_samples(audio_len[row], ld, step);
        const long parts = collect_parts(n, invert);
        __syncthreads();                           // the previous item's readers are done with the tables
        long long total = 0;
        for (long base = 0; base < parts; base += 64) {
            const long k = base + lane;
            Part p{0, 0};
            if (k < parts) p = collect_part(segs + row * cap, n, k, len, invert);
            long long x = p.b > p.a ? p.b - p.a : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long y = __shfl_up(x, (unsigned)d);
                if (lane >= d) x += y;
            }
            if (k < parts) {
                s_incl[k] = total + x;
                s_first[k] = p.a;
            }
            total += __shfl(x, 63);
        }
        __syncthreads();
        const long live = want < total ? want : (long)total;          // (a kept[] that is not this table's never leads outside it)
        const uint8_t *src_row = pcm + row * ld * ESZ;
        uint8_t *dst_row = out + out_offset[row] * ESZ;
        const bool vec_dst = (((size_t)dst_row) & 15) == 0;
        // a row with more tiles than the batch row has samples for (overlapping segments): the item takes them in turn
        for (long tile = tile0; tile * EPT < live; tile += tiles_per_row) {
            long o0[8];
            int part[8], mode[8];                  // 0: nothing, 1: fast, 2: slow
            const uint8_t *sp[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                o0[v] = tile * EPT + (long)(v * 64 + lane) * EPV;
                mode[v] = 0, part[v] = 0, sp[v] = nullptr;
                if (o0[v] >= live) continue;
                int lo = 0, hi = (int)parts - 1;   // the first part whose inclusive sum lies behind o0 (o0 < live <= the last sum)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_incl[mid] > o0[v]) hi = mid;
                    else lo = mid + 1;
                }
                part[v] = lo;
                if (step == 1 && vec_dst && o0[v] + EPV <= s_incl[lo]) {
                    const long long before = lo ? s_incl[lo - 1] : 0;
                    sp[v] = src_row + (s_first[lo] + (o0[v] - before)) * ESZ;
                    mode[v] = 1;
                } else {
                    mode[v] = 2;
                }
            }
            u32x4 c[8], nx[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                if (mode[v] != 1) continue;
                const size_t at = (size_t)sp[v], m = at & 15;
                c[v] = *reinterpret_cast<const u32x4 *>(at - m);
                nx[v] = c[v];
                if (m) nx[v] = *reinterpret_cast<const u32x4 *>(at - m + 16);
            }
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                if (mode[v] == 1) {
                    *reinterpret_cast<u32x4 *>(dst_row + o0[v] * ESZ) = funnel(c[v], nx[v], (int)(((size_t)sp[v]) & 15));
                } else if (mode[v] == 2) {
                    unsigned w[4] = {0u, 0u, 0u, 0u};
                    int p = part[v], got = 0;
#pragma unroll
                    for (int j = 0; j < EPV; ++j) {
                        const long o = o0[v] + j;
                        if (o >= live) continue;
                        while (o >= s_incl[p]) ++p;                       // (o < live: a part behind o exists)
                        const long long before = p ? s_incl[p - 1] : 0;
                        const long long e = (s_first[p] + (o - before)) * step;
                        const unsigned val = *reinterpret_cast<const elem_t *>(src_row + e * ESZ);
                        if (ESZ == 2) w[j >> 1] |= val << (16 * (j & 1));
                        else w[j] = val;
                        got = j + 1;
                    }
                    if (got == EPV && vec_dst) {
                        *reinterpret_cast<u32x4 *>(dst_row + o0[v] * ESZ) = u32x4{w[0], w[1], w[2], w[3]};
                    } else {
#pragma unroll
                        for (int j = 0; j < EPV; ++j) {
                            if (j >= got) continue;
                            const unsigned val = ESZ == 2 ? (w[j >> 1] >> (16 * (j & 1))) & 0xffffu : w[j & 3];
                            *reinterpret_cast<elem_t *>(dst_row + (o0[v] + j) * ESZ) = (elem_t)val;
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_count_kept(long ld, int step, long n_rows, const long *audio_len, const vad_segment *segs, long cap, const long *counts,
                             int invert, long *kept, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(count_kept_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, s, ld, step, n_rows, audio_len, segs, cap,
                       counts, invert, kept);
    return hipGetLastError();
}

hipError_t launch_collect_segments(const void *pcm, int esz, long ld, int step, long n_rows, const long *audio_len, const vad_segment *segs,
                                   long cap, const long *counts, int invert, const long *kept, const long *out_offset, void *out,
                                   hipStream_t s) {
    if (n_rows <= 0 || ld <= 0) return hipSuccess;
    const long samples = (ld + step - 1) / step;               // what a row can keep when its segments do not overlap
    const long tiles = (samples * esz + kTileBytes - 1) / kTileBytes;
    const long items = n_rows * tiles;
    if (items > 0x7fffffffL) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(items < 4096 ? items : 4096);   // HBM to HBM: as wide as the chip (launch_gather_rows)
    const uint8_t *src = static_cast<const uint8_t *>(pcm);
    uint8_t *dst = static_cast<uint8_t *>(out);
    if (esz == 2)
        hipLaunchKernelGGL(collect_segments_kernel<2>, dim3(grid), dim3(64), 0, s, src, ld, step, n_rows, audio_len, segs, cap, counts,
                           invert, kept, out_offset, dst, tiles);
    else
        hipLaunchKernelGGL(collect_segments_kernel<4>, dim3(grid), dim3(64), 0, s, src, ld, step, n_rows, audio_len, segs, cap, counts,
                           invert, kept, out_offset, dst, tiles);
    return hipGetLastError();
}

}  // namespace vad
