// kernel_snapshot.hip -- snapshot and restore of the pump's live streams (vad_pump_export_streams* / vad_pump_import_streams,
// include/silero_vad_hip.h "SNAPSHOT AND RESTORE"; host side: pump.hip).
//
// A stream's carried state lies in several places on the device: h and c in the state block of its PART ([2][hi - lo][128], so its row is
// part-relative), its context in whichever of the two ping-pong buffers the next tick reads, its pending samples in its row of the carry
// and, if it is bound to a resampled rate, its pending fp32 outputs and its filter history in their rows.  Moving 8 192 streams with one
// hipMemcpy per piece is tens of thousands of copies; a drain has to fit between two 32 ms ticks.  So the records are packed (gather) or
// unpacked (scatter) on the device, in the blob's record layout, and ONE copy crosses the link.
//
// ONE RECORD, one wave.  A record is 16-byte vectors, and a lane moves vectors v = lane, lane + 64, ... of it (move_record):
//   [0, 2)            vad_stream_info -- the host's: the gather writes zeros (the host fills it in behind the copy), the scatter skips it
//   [2, 34) h   [34, 66) c   [66, 66 + C / 4) context   [.., .. + N / 8) the pending int16 samples, [0:pending] live
// and, in a record WITH A TAIL (blob versions 2 and 3; TAIL = true), behind them
//   [T, T + 2)        vad_resample_info -- the host's   (T = the vectors above: 146 at 16 kHz, 106 at 8 kHz)
//   [.., .. + N / 4)  the stream's row of the fp32 carry, [0:c] live   [.., .. + 20)  its filter history, int16[160], [0:H] live
//   [.., .. + xv)     extra vectors -- the host's (version 3: the 32 bytes of vad_tape_info)
// Whatever lies behind a live count is zero in a record whatever the device row holds there (the assembly kernels leave their old tails
// in place), and the scatter writes zeros there whatever the record holds: the blob is untrusted, the rows stay canonical.
// The work list is a table the host writes into page-locked mapped memory, read in place like the probabilities are written in place,
// every field range-checked on the host: int4 {slot, part, pending, record} per record, and with a tail a second int4 {c, H, bound, 0}
// behind it.  Without a tail a record costs ONE entry and the kernels know neither the fp32 carry nor the history.  An unbound stream's
// tail is zeros in a record and its scatter leaves the fp32 carry and the history alone (vad_pump_open / close zeroed them); a bound
// stream's scatter writes the WHOLE carry row and the WHOLE history row at the destination's own history pitch, which need not be the
// source's.  The history lies at the start of its row, oldest sample first, where assemble_resampled_packets (kernel_present.hip)
// reads and writes it.  HBM-bound byte movers like expand_rows_kernel: ~19 MB for 8 192 streams at 16 kHz, a few microseconds.
//
// THE RUNS OF THE TAPE (blob version 3) lie behind the records: of each stream whole chunks of its tape (kernel_tape.hip), the newest
// ones, from a position the caller names (tape_run of tape.hpp).  move_runs below moves them between a stream's ring and a staging
// buffer that holds the runs packed in record order -- the blob's tape section, which crosses the link in one copy.
#include <hip/hip_runtime.h>

#include "device_api.hpp"
#include "tape.hpp"

namespace vad {
namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));
using i16x8 = short __attribute__((ext_vector_type(8)));
constexpr int kSnapWaves = 4;                    // records per workgroup
constexpr int kInfoVec = 2, kStateVec = 128 / 4; // 16-byte vectors of the info block, of h and of c
constexpr int kTailInfoVec = 2, kTailHistVec = kSnapHistory / 8;     // 16-byte vectors of vad_resample_info and of history[160]

// int16 samples [8 j, 8 j + 8) of a row, zeros from sample `pending` on -- the only place that zeroes behind a live count; nothing is read
// of a vector that lies behind it.  (fp32 rows go through it with twice their count: +0.0f is two zero samples.)
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

// The walk of one record, and the one place that knows its vector map: for the part a vector lies in, which vector j of the part it is,
// the device row the part mirrors and how many int16s of that row are live (kWhole: a part without a count; the host's parts: no row,
// nothing live, so zeros).  One load, pending_vec and one store then move the vector in either direction.  The gather walks every vector
// of the record; the scatter walks the vectors of the slot -- none of the host's, the history at the slot's own pitch hv, zeros behind
// the record's 20 vectors of it -- and leaves the tail of an unbound record alone.  F4 / I8 / R4: f32x4 / i16x8 / f32x4, const on the
// side the direction reads.  fv, hv, xv (TAIL): the vectors of a row of the fp32 carry, of a row of `hist`, and the extra ones behind
// the record's history.
constexpr int kWhole = 0x7fffffff;

template <bool TAIL, bool SCATTER, class F4, class I8, class R4>
__device__ __forceinline__ void move_record(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts, F4 *__restrict__ ctx,
                                            I8 *__restrict__ carry, F4 *__restrict__ fcarry, I8 *__restrict__ hist, int cv, int nv, int fv, int hv, int xv,
                                            R4 *__restrict__ rec) {
    const long i = (long)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int4 e = table[TAIL ? 2 * i : i];      // {slot, part, pending, record}
    int4 t = {};                                 // {c, H, bound, 0}
    if constexpr (TAIL) t = table[2 * i + 1];
    const SnapPart pt = parts[e.y];
    const size_t row = (size_t)(e.x - pt.lo);
    const int at_c = kInfoVec + kStateVec, at_ctx = at_c + kStateVec, at_pending = at_ctx + cv, at_tail = at_pending + nv;
    const int at_fcarry = at_tail + kTailInfoVec, at_hist = at_fcarry + fv, at_extra = at_hist + kTailHistVec;
    const int stride = TAIL ? at_extra + xv : at_tail;
    auto *r16 = reinterpret_cast<std::conditional_t<SCATTER, const i16x8, i16x8> *>(rec + (size_t)e.w * stride);
    const int end = !SCATTER ? stride : TAIL && t.z ? at_hist + hv : at_tail;
    for (int v = (SCATTER ? kInfoVec : 0) + lane; v < end; v += 64) {
        int j = 0, live = 0;
        I8 *dev = nullptr;
        if (TAIL && !SCATTER && v >= at_extra) ;                                                                    // the host's
        else if (TAIL && v >= at_hist) j = v - at_hist, dev = hist + (size_t)e.x * hv, live = t.z && v < at_extra ? t.y : 0;
        else if (TAIL && v >= at_fcarry) j = v - at_fcarry, dev = reinterpret_cast<I8 *>(fcarry + (size_t)e.x * fv), live = t.z ? 2 * t.x : 0;
        else if (TAIL && v >= at_tail) ;                                                                            // the host's
        else if (v >= at_pending) j = v - at_pending, dev = carry + (size_t)e.x * nv, live = e.z;
        else if (v >= at_ctx) j = v - at_ctx, dev = reinterpret_cast<I8 *>(ctx + (size_t)e.x * cv), live = kWhole;
        else if (v >= at_c) j = v - at_c, dev = reinterpret_cast<I8 *>(pt.state + ((size_t)pt.n + row) * 128), live = kWhole;
        else if (v >= kInfoVec) j = v - kInfoVec, dev = reinterpret_cast<I8 *>(pt.state + row * 128), live = kWhole;
        if (SCATTER && !dev) continue;
        // the vector itself and what is live from it on (an unbound stream: fcarry / hist may be null -- nothing of them is live, nothing is read)
        const i16x8 x = pending_vec(SCATTER ? r16 + v : dev + j, 0, live - 8 * j);
        if constexpr (SCATTER) dev[j] = x;
        else r16[v] = x;
    }
}

template <bool TAIL>
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_gather_kernel(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts,
                                                                          const f32x4 *__restrict__ ctx, const i16x8 *__restrict__ carry,
                                                                          const f32x4 *__restrict__ fcarry, const i16x8 *__restrict__ hist, int cv, int nv,
                                                                          int fv, int hv, int xv, f32x4 *__restrict__ rec) {
    move_record<TAIL, false>(table, n, parts, ctx, carry, fcarry, hist, cv, nv, fv, hv, xv, rec);
}

template <bool TAIL>
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_scatter_kernel(const int4 *__restrict__ table, long n, const SnapPart *__restrict__ parts,
                                                                           f32x4 *__restrict__ ctx, i16x8 *__restrict__ carry, f32x4 *__restrict__ fcarry,
                                                                           i16x8 *__restrict__ hist, int cv, int nv, int fv, int hv, int xv,
                                                                           const f32x4 *__restrict__ rec) {
    move_record<TAIL, true>(table, n, parts, ctx, carry, fcarry, hist, cv, nv, fv, hv, xv, rec);
}

// The runs of the tape.  One item = (run r, group g): chunks [4 g, 4 g + 4) of the run, one wave; the items of a launch are
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

// (from, to) = (the tape, the packed runs)
template <int ELEM>
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_tape_gather_kernel(const SnapRun *__restrict__ runs, long n_runs, long groups,
                                                                               const u32x4 *__restrict__ from, int chunks, int rv, u32x4 *__restrict__ to) {
    move_runs<ELEM, false>(runs, n_runs, groups, from, chunks, rv, to);
}

// (from, to) = (the packed runs, the tape)
template <int ELEM>
__global__ void __launch_bounds__(64 * kSnapWaves) snapshot_tape_scatter_kernel(const SnapRun *__restrict__ runs, long n_runs, long groups,
                                                                                const u32x4 *__restrict__ from, int chunks, int rv, u32x4 *__restrict__ to) {
    move_runs<ELEM, true>(runs, n_runs, groups, from, chunks, rv, to);
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

// Both directions' launch.  F / I / R: float / int16_t / uint8_t, const on the side the direction reads.  tail: null for records without one.
template <bool SCATTER, class F, class I, class R>
hipError_t launch_records(const int32_t *table, long n, const SnapPart *parts, F *ctx, I *carry, int N, int C, R *records, hipStream_t s, const SnapTail *tail) {
    using F4 = std::conditional_t<SCATTER, f32x4, const f32x4>;
    using I8 = std::conditional_t<SCATTER, i16x8, const i16x8>;
    using R4 = std::conditional_t<SCATTER, const f32x4, f32x4>;
    if (n <= 0) return hipSuccess;
    if (!snap_args_ok(table, parts, ctx, carry, N, C, records) ||
        (tail && (!snap_tail_ok(tail->fcarry, tail->hist, tail->hist_ld) || tail->extra_bytes < 0 || tail->extra_bytes % 16)))
        return hipErrorInvalidValue;
    const SnapTail tl = tail ? *tail : SnapTail{};
    void (*kernel)(const int4 *, long, const SnapPart *, F4 *, I8 *, F4 *, I8 *, int, int, int, int, int, R4 *);
    if constexpr (SCATTER) kernel = tail ? snapshot_scatter_kernel<true> : snapshot_scatter_kernel<false>;
    else kernel = tail ? snapshot_gather_kernel<true> : snapshot_gather_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + kSnapWaves - 1) / kSnapWaves)), dim3(64 * kSnapWaves), 0, s, reinterpret_cast<const int4 *>(table), n, parts,
                       reinterpret_cast<F4 *>(ctx), reinterpret_cast<I8 *>(carry), reinterpret_cast<F4 *>(tl.fcarry), reinterpret_cast<I8 *>(tl.hist), C / 4,
                       N / 8, N / 4, tl.hist ? tl.hist_ld / 8 : 0, tl.extra_bytes / 16, reinterpret_cast<R4 *>(records));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_snapshot_gather(const int32_t *table, long n, const SnapPart *parts, const float *ctx, const int16_t *carry, int N, int C,
                                  uint8_t *records, hipStream_t s, const SnapTail *tail) {
    return launch_records<false>(table, n, parts, ctx, carry, N, C, records, s, tail);
}

hipError_t launch_snapshot_scatter(const int32_t *table, long n, const SnapPart *parts, float *ctx, int16_t *carry, int N, int C,
                                   const uint8_t *records, hipStream_t s, const SnapTail *tail) {
    return launch_records<true>(table, n, parts, ctx, carry, N, C, records, s, tail);
}

hipError_t launch_snapshot_tape(bool scatter, const SnapRun *runs, long n_runs, long max_n, void *tape, int chunks, int N, int elem, void *packed,
                                hipStream_t s) {
    long groups = 0;
    const long grid = snap_runs_grid(runs, n_runs, max_n, tape, chunks, N, elem, packed, &groups);
    if (grid <= 0) return grid ? hipErrorInvalidValue : hipSuccess;
    const auto kernel = scatter ? (elem == 2 ? snapshot_tape_scatter_kernel<2> : snapshot_tape_scatter_kernel<4>)
                                : (elem == 2 ? snapshot_tape_gather_kernel<2> : snapshot_tape_gather_kernel<4>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * kSnapWaves), 0, s, runs, n_runs, groups, static_cast<const u32x4 *>(scatter ? packed : tape),
                       chunks, N * elem / 16, static_cast<u32x4 *>(scatter ? tape : packed));
    return hipGetLastError();
}

}  // namespace vad
