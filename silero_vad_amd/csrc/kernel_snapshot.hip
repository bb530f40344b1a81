// kernel_snapshot.hip -- snapshot and restore of the pump's live streams (vad_pump_export_streams / vad_pump_import_streams,
// include/silero_vad_hip.h "SNAPSHOT AND RESTORE"; host side: pump.hip).
//
// A stream's carried state lies in four places on the device: h and c in the state block of its PART ([2][hi - lo][128], so its row is
// part-relative), its context in whichever of the two ping-pong buffers the next tick reads, its pending samples in its row of the carry.
// Moving 8 192 streams with one hipMemcpy per piece is tens of thousands of copies; a drain has to fit between two 32 ms ticks.  So the
// records are packed (gather) or unpacked (scatter) on the device, in the blob's record layout, and ONE copy crosses the link.
//
// One wave per record; a lane moves 16-byte vectors v = lane, lane + 64, ... of the record (146 at 16 kHz, 106 at 8 kHz):
//   [0, 2)  vad_stream_info: host bookkeeping -- the gather writes zeros (the host fills it in behind the copy), the scatter skips it
//   [2, 34) h   [34, 66) c   [66, 66 + C / 4) context   [66 + C / 4, ... + N / 8) the pending samples
// Samples behind the stream's pending count are zero in a record whatever the carry holds there (the assembly kernels leave their old
// tails in place), and the scatter writes them as zeros whatever the record holds: the blob is untrusted, the carry stays canonical.
// The work list is a table of int4 {slot, part, pending, record} the host writes into page-locked mapped memory (16 bytes a record,
// read in place like the probabilities are written in place); every field of it was range-checked on the host.  HBM-bound byte movers
// like expand_rows_kernel: ~19 MB for 8 192 streams at 16 kHz, a few microseconds.
#include <hip/hip_runtime.h>

#include "device_api.hpp"

namespace vad {
namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));
using i16x8 = short __attribute__((ext_vector_type(8)));
constexpr int kSnapWaves = 4;                    // records per workgroup
constexpr int kInfoVec = 2, kStateVec = 128 / 4; // 16-byte vectors of the info block, of h and of c

// the stream's pending samples [8 j, 8 j + 8) of a row, zeros from sample `pending` on
__device__ inline i16x8 pending_vec(const i16x8 *__restrict__ row, int j, int pending) {
    i16x8 s = {};
    if (8 * j < pending) {
        s = row[j];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (8 * j + k >= pending) s[k] = 0;
    }
    return s;
}

__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_gather_kernel(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts,
                                                                          const f32x4 *__restrict__ ctx, const i16x8 *__restrict__ carry, int cv, int nv,
                                                                          f32x4 *__restrict__ rec) {
    const long i = (long)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int4 e = table[i];
    const SnapPart pt = parts[e.y];
    const size_t row = (size_t)(e.x - pt.lo);
    const f32x4 *h = reinterpret_cast<const f32x4 *>(pt.state + row * 128), *c = reinterpret_cast<const f32x4 *>(pt.state + ((size_t)pt.n + row) * 128);
    const int total = kInfoVec + 2 * kStateVec + cv + nv;
    f32x4 *out = rec + (size_t)e.w * total;
    for (int v = lane; v < total; v += 64) {
        const int u = v - kInfoVec - 2 * kStateVec;
        if (u >= cv) {
            reinterpret_cast<i16x8 *>(out)[v] = pending_vec(carry + (size_t)e.x * nv, u - cv, e.z);
            continue;
        }
        f32x4 x = {};
        if (u >= 0) x = ctx[(size_t)e.x * cv + u];
        else if (v >= kInfoVec + kStateVec) x = c[v - kInfoVec - kStateVec];
        else if (v >= kInfoVec) x = h[v - kInfoVec];
        out[v] = x;
    }
}

__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_scatter_kernel(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts,
                                                                           f32x4 *__restrict__ ctx, i16x8 *__restrict__ carry, int cv, int nv,
                                                                           const f32x4 *__restrict__ rec) {
    const long i = (long)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int4 e = table[i];
    const SnapPart pt = parts[e.y];
    const size_t row = (size_t)(e.x - pt.lo);
    f32x4 *h = reinterpret_cast<f32x4 *>(pt.state + row * 128), *c = reinterpret_cast<f32x4 *>(pt.state + ((size_t)pt.n + row) * 128);
    const int total = kInfoVec + 2 * kStateVec + cv + nv;
    const f32x4 *in = rec + (size_t)e.w * total;
    for (int v = kInfoVec + lane; v < total; v += 64) {
        const int u = v - kInfoVec - 2 * kStateVec;
        if (u >= cv) carry[(size_t)e.x * nv + (u - cv)] = pending_vec(reinterpret_cast<const i16x8 *>(in) + (kInfoVec + 2 * kStateVec + cv), u - cv, e.z);
        else if (u >= 0) ctx[(size_t)e.x * cv + u] = in[v];
        else if (v >= kInfoVec + kStateVec) c[v - kInfoVec - kStateVec] = in[v];
        else h[v - kInfoVec] = in[v];
    }
}

bool snap_args_ok(const int32_t *table, const SnapPart *parts, const void *ctx, const void *carry, int N, int C, const void *records) {
    return table && parts && ctx && carry && records && N > 0 && N % 8 == 0 && C > 0 && C % 4 == 0;
}

}  // namespace

hipError_t launch_snapshot_gather(const int32_t *table, long n, const SnapPart *parts, const float *ctx, const int16_t *carry, int N, int C,
                                  uint8_t *records, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!snap_args_ok(table, parts, ctx, carry, N, C, records)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snapshot_gather_kernel, dim3((unsigned)((n + kSnapWaves - 1) / kSnapWaves)), dim3(64 * kSnapWaves), 0, s,
                       reinterpret_cast<const int4 *>(table), n, parts, reinterpret_cast<const f32x4 *>(ctx), reinterpret_cast<const i16x8 *>(carry),
                       C / 4, N / 8, reinterpret_cast<f32x4 *>(records));
    return hipGetLastError();
}

hipError_t launch_snapshot_scatter(const int32_t *table, long n, const SnapPart *parts, float *ctx, int16_t *carry, int N, int C,
                                   const uint8_t *records, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!snap_args_ok(table, parts, ctx, carry, N, C, records)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snapshot_scatter_kernel, dim3((unsigned)((n + kSnapWaves - 1) / kSnapWaves)), dim3(64 * kSnapWaves), 0, s,
                       reinterpret_cast<const int4 *>(table), n, parts, reinterpret_cast<f32x4 *>(ctx), reinterpret_cast<i16x8 *>(carry), C / 4, N / 8,
                       reinterpret_cast<const f32x4 *>(records));
    return hipGetLastError();
}

}  // namespace vad
