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
//
// Blob version 2 (vad_pump_export_streams_v2) carries a stream that is BOUND to a resampled rate as well.  Its record is the version 1
// record followed by a tail, and the gather2 / scatter2 kernels are the same wave walking further vectors of a longer record:
//   [T, T + 2)  vad_resample_info: host bookkeeping like the info block   (T = the vectors of a version 1 record)
//   [T + 2, T + 2 + N / 4)  the stream's row of the fp32 carry, [0:c] live   [.., .. + 20)  its filter history, int16[160], [0:H] live
// The work list has TWO int4 per record there: the entry above and {c, H, bound, 0}.  An unbound stream's tail is zeros in a record and
// its scatter leaves the fp32 carry and the history alone (vad_pump_open / close zeroed them); a bound stream's scatter writes the WHOLE
// carry row and the WHOLE history row -- zeros behind c and behind H whatever the record and the slot held -- at the destination's own
// history pitch, which need not be the source's.  The history lies at the start of its row, oldest sample first, where
// assemble_resampled_packets (kernel_present.hip) reads and writes it.
//
// Blob version 3 (vad_pump_export_streams_v3) carries, behind the records, a RUN of each stream's tape (kernel_tape.hip): whole chunks,
// the newest ones, from a position the caller names (tape_run of tape.hpp).  Its record is the version 2 record followed by the 32 bytes
// of vad_tape_info, the host's: gather2 / scatter2 take the count of such extra vectors, write them as zeros and skip them.  The runs
// themselves are moved by snapshot_tape_gather_kernel / snapshot_tape_scatter_kernel below, between a stream's ring and a staging buffer
// that holds the runs packed in record order -- the blob's tape section, which crosses the link in one copy.
#include <hip/hip_runtime.h>

#include "device_api.hpp"
#include "tape.hpp"

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

// the same for fp32 outputs: floats [4 j, 4 j + 4) of a row, +0.0f from float `live` on
__device__ inline f32x4 live_vec(const f32x4 *__restrict__ row, int j, int live) {
    f32x4 s = {};
    if (4 * j < live) {
        s = row[j];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * j + k >= live) s[k] = 0.0f;
    }
    return s;
}

constexpr int kTailInfoVec = 2, kTailHistVec = kSnapHistory / 8;     // 16-byte vectors of vad_resample_info and of history[160]

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

// Version 2: the version 1 vectors exactly as above, then the tail.  t = {c, H, bound, 0} of the record's second table entry.
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_gather2_kernel(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts,
                                                                           const f32x4 *__restrict__ ctx, const i16x8 *__restrict__ carry,
                                                                           const f32x4 *__restrict__ fcarry, const i16x8 *__restrict__ hist, int cv, int nv,
                                                                           int fv, int hv, int xv, f32x4 *__restrict__ rec) {
    const long i = (long)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int4 e = table[2 * i], t = table[2 * i + 1];
    const SnapPart pt = parts[e.y];
    const size_t row = (size_t)(e.x - pt.lo);
    const f32x4 *h = reinterpret_cast<const f32x4 *>(pt.state + row * 128), *c = reinterpret_cast<const f32x4 *>(pt.state + ((size_t)pt.n + row) * 128);
    const int v1 = kInfoVec + 2 * kStateVec + cv + nv, v2 = v1 + kTailInfoVec + fv + kTailHistVec, total = v2 + xv;
    const int live = t.z ? t.x : 0, H = t.z ? t.y : 0;         // (an unbound stream: fcarry / hist may be null, and are not read)
    f32x4 *out = rec + (size_t)e.w * total;
    for (int v = lane; v < total; v += 64) {
        if (v >= v1) {                           // the tail: zeros for the host's block, the live carry, the live history; zeros for the xv vectors behind it
            const int w = v - v1 - kTailInfoVec;
            if (v >= v2) out[v] = f32x4{};
            else if (w >= fv) reinterpret_cast<i16x8 *>(out)[v] = pending_vec(hist + (size_t)e.x * hv, w - fv, H);
            else out[v] = w >= 0 ? live_vec(fcarry + (size_t)e.x * fv, w, live) : f32x4{};
            continue;
        }
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

// hv: the DESTINATION's history pitch in vectors.  A bound record writes carry vectors [0, fv) and history vectors [0, hv) of the slot.
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_scatter2_kernel(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts,
                                                                            f32x4 *__restrict__ ctx, i16x8 *__restrict__ carry, f32x4 *__restrict__ fcarry,
                                                                            i16x8 *__restrict__ hist, int cv, int nv, int fv, int hv, int xv,
                                                                            const f32x4 *__restrict__ rec) {
    const long i = (long)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int4 e = table[2 * i], t = table[2 * i + 1];
    const SnapPart pt = parts[e.y];
    const size_t row = (size_t)(e.x - pt.lo);
    f32x4 *h = reinterpret_cast<f32x4 *>(pt.state + row * 128), *c = reinterpret_cast<f32x4 *>(pt.state + ((size_t)pt.n + row) * 128);
    const int v1 = kInfoVec + 2 * kStateVec + cv + nv, stride = v1 + kTailInfoVec + fv + kTailHistVec + xv;
    const f32x4 *in = rec + (size_t)e.w * stride;
    for (int v = kInfoVec + lane; v < v1; v += 64) {
        const int u = v - kInfoVec - 2 * kStateVec;
        if (u >= cv) carry[(size_t)e.x * nv + (u - cv)] = pending_vec(reinterpret_cast<const i16x8 *>(in) + (kInfoVec + 2 * kStateVec + cv), u - cv, e.z);
        else if (u >= 0) ctx[(size_t)e.x * cv + u] = in[v];
        else if (v >= kInfoVec + kStateVec) c[v - kInfoVec - kStateVec] = in[v];
        else h[v - kInfoVec] = in[v];
    }
    if (!t.z) return;                            // an unbound record: the slot's fp32 carry and history stay as they are
    const f32x4 *in_carry = in + v1 + kTailInfoVec;
    const i16x8 *in_hist = reinterpret_cast<const i16x8 *>(in_carry + fv);
    for (int w = lane; w < fv + hv; w += 64) {
        if (w < fv) fcarry[(size_t)e.x * fv + w] = live_vec(in_carry, w, t.x);
        else hist[(size_t)e.x * hv + (w - fv)] = pending_vec(in_hist, w - fv, w - fv < kTailHistVec ? t.y : 0);
    }
}

// Version 3: the runs of the tape.  One item = (run r, group g): chunks [4 g, 4 g + 4) of the run, one wave; the items of a launch are
// n_runs x groups (groups = the longest run's), dealt over a grid-stride loop, and a group behind its run's last chunk is left at once.
// A row is rv = N * ELEM / 16 vectors (32 ... 128): lane l moves vectors l and, on the fp32 tape, l + 64 of each of the group's rows --
// every one an aligned 16-byte load and an aligned 16-byte store, all of the item's loads in front of its first store.  The run's entry is
// wave-uniform and read in place from the host's mapped table.  SCATTER: the same walk with the two sides exchanged.
constexpr int kRunGroup = 4;
using u32x4 = unsigned __attribute__((ext_vector_type(4)));

template <int ELEM, bool SCATTER>
__device__ __forceinline__ void move_runs(const SnapRun *__restrict__ runs, long n_runs, long groups, const u32x4 *__restrict__ from, int chunks, int rv,
                                          u32x4 *__restrict__ to) {
    constexpr int W = ELEM / 2;                  // vectors of a row a lane moves
    const int lane = threadIdx.x & 63;
    const long items = n_runs * groups;
    for (long item = (long)blockIdx.x * kSnapWaves + (threadIdx.x >> 6); item < items; item += (long)gridDim.x * kSnapWaves) {
        const long r = item / groups, k0 = item % groups * kRunGroup;
        const SnapRun q = runs[r];
        if (k0 >= q.n) continue;
        const unsigned s0 = (unsigned)tape_slot(q.first + k0, chunks);
        size_t ring[kRunGroup], pack[kRunGroup];   // the rows' first vectors on the tape and in the packed runs
        u32x4 x[kRunGroup][W];
#pragma unroll
        for (int j = 0; j < kRunGroup; ++j) {
            ring[j] = ((size_t)q.slot * chunks + (s0 + j) % (unsigned)chunks) * rv;
            pack[j] = (size_t)(q.at + k0 + j) * rv;
        }
#pragma unroll
        for (int j = 0; j < kRunGroup; ++j)
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (k0 + j < q.n && lane + 64 * w < rv) x[j][w] = from[(SCATTER ? pack[j] : ring[j]) + lane + 64 * w];
#pragma unroll
        for (int j = 0; j < kRunGroup; ++j)
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (k0 + j < q.n && lane + 64 * w < rv) to[(SCATTER ? ring[j] : pack[j]) + lane + 64 * w] = x[j][w];
    }
}

template <int ELEM>
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_tape_gather_kernel(const SnapRun *__restrict__ runs, long n_runs, long groups,
                                                                               const u32x4 *__restrict__ tape, int chunks, int rv, u32x4 *__restrict__ packed) {
    move_runs<ELEM, false>(runs, n_runs, groups, tape, chunks, rv, packed);
}

template <int ELEM>
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_tape_scatter_kernel(const SnapRun *__restrict__ runs, long n_runs, long groups,
                                                                                u32x4 *__restrict__ tape, int chunks, int rv, const u32x4 *__restrict__ packed) {
    move_runs<ELEM, true>(runs, n_runs, groups, packed, chunks, rv, tape);
}

// -> the launch's grid (0: nothing to do), or -1 for arguments no launch may have
long snap_runs_grid(const SnapRun *runs, long n_runs, long max_n, const void *tape, int chunks, int N, int elem, const void *packed, long *groups) {
    if (n_runs <= 0 || max_n <= 0) return 0;
    if (!runs || !tape || !packed || (((size_t)tape | (size_t)packed) & 15) || (elem != 2 && elem != 4) || N < 8 || N % 8 || N * elem / 16 > 32 * elem ||
        chunks < 1 || max_n > chunks)
        return -1;
    *groups = (max_n + kRunGroup - 1) / kRunGroup;
    if (n_runs > 0x7fffffffL / *groups) return -1;
    const long blocks = (n_runs * *groups + kSnapWaves - 1) / kSnapWaves;
    return blocks < 8192 ? blocks : 8192;        // HBM to HBM: as wide as the chip, the rest by the loop
}

bool snap_args_ok(const int32_t *table, const SnapPart *parts, const void *ctx, const void *carry, int N, int C, const void *records) {
    return table && parts && ctx && carry && records && N > 0 && N % 8 == 0 && C > 0 && C % 4 == 0;
}

// (a pump without the resampled route has neither buffer: its table then holds no bound entry, and the kernels touch neither)
bool snap_tail_ok(const void *fcarry, const void *hist, int hist_ld) { return (fcarry && hist && hist_ld > 0 && hist_ld % 8 == 0) || (!fcarry && !hist); }

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

hipError_t launch_snapshot_gather2(const int32_t *table, long n, const SnapPart *parts, const float *ctx, const int16_t *carry, const float *fcarry,
                                   const int16_t *hist, int hist_ld, int N, int C, uint8_t *records, hipStream_t s, int extra_bytes) {
    if (n <= 0) return hipSuccess;
    if (!snap_args_ok(table, parts, ctx, carry, N, C, records) || !snap_tail_ok(fcarry, hist, hist_ld) || extra_bytes < 0 || extra_bytes % 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snapshot_gather2_kernel, dim3((unsigned)((n + kSnapWaves - 1) / kSnapWaves)), dim3(64 * kSnapWaves), 0, s,
                       reinterpret_cast<const int4 *>(table), n, parts, reinterpret_cast<const f32x4 *>(ctx), reinterpret_cast<const i16x8 *>(carry),
                       reinterpret_cast<const f32x4 *>(fcarry), reinterpret_cast<const i16x8 *>(hist), C / 4, N / 8, N / 4, hist ? hist_ld / 8 : 0, extra_bytes / 16,
                       reinterpret_cast<f32x4 *>(records));
    return hipGetLastError();
}

hipError_t launch_snapshot_scatter2(const int32_t *table, long n, const SnapPart *parts, float *ctx, int16_t *carry, float *fcarry, int16_t *hist,
                                    int hist_ld, int N, int C, const uint8_t *records, hipStream_t s, int extra_bytes) {
    if (n <= 0) return hipSuccess;
    if (!snap_args_ok(table, parts, ctx, carry, N, C, records) || !snap_tail_ok(fcarry, hist, hist_ld) || extra_bytes < 0 || extra_bytes % 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snapshot_scatter2_kernel, dim3((unsigned)((n + kSnapWaves - 1) / kSnapWaves)), dim3(64 * kSnapWaves), 0, s,
                       reinterpret_cast<const int4 *>(table), n, parts, reinterpret_cast<f32x4 *>(ctx), reinterpret_cast<i16x8 *>(carry),
                       reinterpret_cast<f32x4 *>(fcarry), reinterpret_cast<i16x8 *>(hist), C / 4, N / 8, N / 4, hist ? hist_ld / 8 : 0, extra_bytes / 16,
                       reinterpret_cast<const f32x4 *>(records));
    return hipGetLastError();
}

hipError_t launch_snapshot_tape_gather(const SnapRun *runs, long n_runs, long max_n, const void *tape, int chunks, int N, int elem, void *packed,
                                       hipStream_t s) {
    long groups = 0;
    const long grid = snap_runs_grid(runs, n_runs, max_n, tape, chunks, N, elem, packed, &groups);
    if (grid <= 0) return grid ? hipErrorInvalidValue : hipSuccess;
    const u32x4 *from = static_cast<const u32x4 *>(tape);
    u32x4 *to = static_cast<u32x4 *>(packed);
    if (elem == 2)
        hipLaunchKernelGGL(snapshot_tape_gather_kernel<2>, dim3((unsigned)grid), dim3(64 * kSnapWaves), 0, s, runs, n_runs, groups, from, chunks, N * elem / 16, to);
    else
        hipLaunchKernelGGL(snapshot_tape_gather_kernel<4>, dim3((unsigned)grid), dim3(64 * kSnapWaves), 0, s, runs, n_runs, groups, from, chunks, N * elem / 16, to);
    return hipGetLastError();
}

hipError_t launch_snapshot_tape_scatter(const SnapRun *runs, long n_runs, long max_n, void *tape, int chunks, int N, int elem, const void *packed,
                                        hipStream_t s) {
    long groups = 0;
    const long grid = snap_runs_grid(runs, n_runs, max_n, tape, chunks, N, elem, packed, &groups);
    if (grid <= 0) return grid ? hipErrorInvalidValue : hipSuccess;
    u32x4 *to = static_cast<u32x4 *>(tape);
    const u32x4 *from = static_cast<const u32x4 *>(packed);
    if (elem == 2)
        hipLaunchKernelGGL(snapshot_tape_scatter_kernel<2>, dim3((unsigned)grid), dim3(64 * kSnapWaves), 0, s, runs, n_runs, groups, to, chunks, N * elem / 16, from);
    else
        hipLaunchKernelGGL(snapshot_tape_scatter_kernel<4>, dim3((unsigned)grid), dim3(64 * kSnapWaves), 0, s, runs, n_runs, groups, to, chunks, N * elem / 16, from);
    return hipGetLastError();
}

}  // namespace vad
