// kernel_present.hip -- live streams that have no chunk this tick (vad_step_present, include/silero_vad_hip.h).
//
// In the reference a stream's (h, c) and context change only when THAT stream's caller calls the model: VADIterator.__call__ runs
// one model call per chunk that arrived (src/silero_vad/utils_vad.py:507-549), the model object replaces _state / _context inside
// that call and nowhere else (JIT!/vad/model/vad_annotator.py:72,86-87), and the native loop does the same around session.run
// (examples/cpp/silero-vad-onnx.cpp:335-390).  A lock-step batch of thousands of live streams has rows whose packet is late: those
// rows must come out of the tick exactly as they went in.
//
// Division of labour.  The step kernels (kernel_front_lat.hip fused step, kernel_rec*.hip) take `present[B]` and simply do not write
// an absent row's (h, c) or probability -- one byte load per lane, nothing when the pointer is null.  The frontends know nothing about
// presence: they write the next context of EVERY row into the second context buffer (ctx_out is never the buffer they read), so an
// absent row's ctx_out holds the tail of whatever its PCM slot held.  This pass runs behind them on the same stream and finishes the
// absent rows: ctx_out[b] = ctx_in[b] (bit copy), probs[b] = VAD_PROB_ABSENT.  HBM-bound byte work: B * C * 4 bytes at most (2 MiB for
// 8 192 streams), one 16-byte vector per lane, rows of present streams are not touched.
//
// expand_rows (compact ticks of the pump, pump.hip): the delivering streams' chunks crossed the link back to back; this pass copies row
// pos[b] of that block to row b of the batch buffer the step kernels read -- HBM-bound byte work, 2 x B x N x 2 bytes at most.
//
// assemble_packets (packet ticks of the pump, pump.hip): receive paths deliver 10 / 20 / 30 ms frames, not 32 ms chunks.  The packets of
// a tick crossed the link back to back (each starting on a 16-byte boundary); a device carry buffer [streams][N] holds what every stream
// has pending.  A stream whose pending samples plus its packet reach N gets its batch row spliced together here (carry ++ packet head)
// and keeps the packet's tail as its new carry; any other stream appends its packet to its carry.  The reference's VADIterator takes
// one chunk per call (utils_vad.py:507-549): a packet stream is the concatenation of its packets, cut into chunks.  HBM-bound byte work:
// 16-byte global loads and stores only, the splice at the unaligned pending length done in LDS.
//
// assemble_coded_packets (packet ticks with G.711 rows, vad_pump_submit_coded_packets): the same splice, with mu-law / A-law rows
// crossing the link at 1 byte a sample and expanded to int16 in registers between their 16-byte load and the LDS row.  Ticks with
// only int16 rows keep taking assemble_packets.
//
// assemble_wide_packets (wide packet ticks, vad_pump_submit_wide_packets): the same splice, with int16 rows sampled at 32 / 48 kHz (WebRTC,
// Opus decoders) decimated to 16 kHz by the reference's rule x[::step] (utils_vad.py:39-42, :301-304) between their 16-byte loads and the
// LDS row.  The comb's phase is carried per stream by the host and arrives in the row table.  Ticks of the other routes never take it.
//
// assemble_resampled_packets (resampled packet ticks, vad_pump_submit_resampled_packets): int16 rows at 44.1 / 24 / 22.05 kHz ... pass the
// streaming form of kernel_resample.hip's polyphase filter on their way into the stream's fp32 chunk; the stream's last K - 1 input
// samples and its fp32 pending outputs are carried on the device, every index comes from the host's row table.  Described at the kernel.
//
// SILENT rows (VAD_ROW_SILENT, every assembly kernel; the resampled one stages zeros in place of the row): a row that stands for `len` samples of digital silence and has no bytes in the
// slot -- a lost packet, a DTX / comfort-noise period.  The table carries the marker where a payload row carries its offset: the offset
// column (table[i].y) holds VAD_ROW_SILENT (-1), every payload offset is >= 0, and the length word keeps its fields (len, kCodecShift,
// kCombShift) with the meanings they have; the host writes VAD_PCM_S16 into the codec field of a silent row, so a G.711 tick never
// expands a zero register (mu-law 0x00 is -32124).  A lane's vector starts as {} and a silent row simply does not overwrite it: one
// compare of the offset per row, uniform across the wave, in front of the guarded load; no address is formed from the marker that is
// dereferenced.  The zeros are spliced at the unaligned pending length like samples.
#include <hip/hip_runtime.h>

#include "adpcm.hpp"
#include "device_api.hpp"

namespace vad {
namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));

// one thread per 16 bytes of context: C / 4 threads per row (16 or 8), 256 threads per workgroup
__global__ void __launch_bounds__(256) carry_absent_kernel(const uint8_t *__restrict__ present, const float *__restrict__ ctx_in,
                                                           float *__restrict__ ctx_out, int vec_per_row, float *__restrict__ probs, long ldp, int B) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long b = i / vec_per_row;
    const int v = (int)(i - b * vec_per_row);
    if (b >= B || present[b]) return;
    const size_t off = (size_t)b * vec_per_row + v;
    if (ctx_out != nullptr) reinterpret_cast<f32x4 *>(ctx_out)[off] = reinterpret_cast<const f32x4 *>(ctx_in)[off];     // (null: the step kernel left the absent rows' context where it was)
    if (v == 0) probs[(size_t)b * ldp] = VAD_PROB_ABSENT;
}

// one thread per 16 bytes of a row: dst[b] <- src[pos[b]] for the rows that deliver (a compact tick of the pump: the link carried only
// those rows, back to back; the step kernels read row b of the batch buffer)
__global__ void __launch_bounds__(256) expand_rows_kernel(const uint8_t *__restrict__ present, const int32_t *__restrict__ pos,
                                                          const f32x4 *__restrict__ src, f32x4 *__restrict__ dst, int vec_per_row, int B) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long b = i / vec_per_row;
    const int v = (int)(i - b * vec_per_row);
    if (b >= B || !present[b]) return;
    dst[(size_t)b * vec_per_row + v] = __builtin_nontemporal_load(src + (size_t)pos[b] * vec_per_row + v);
}

// one wave per packet row, four rows per workgroup.  Each lane moves one 16-byte vector of the carry, of the packet and of the output
// (N / 8 <= 64 vectors each).  The carry is updated in place: the wave's reads of its row finish before the first barrier, its writes
// come after the second, and no other wave touches that row (one packet per stream and tick).
using i16x8 = short __attribute__((ext_vector_type(8)));
constexpr int kPacketRowsPerBlock = 4;

__global__ void __launch_bounds__(64 * kPacketRowsPerBlock) assemble_packets_kernel(const int4 *__restrict__ table, long n_rows,
                                                                                     const int16_t *__restrict__ pkt, int16_t *carry,
                                                                                     i16x8 *__restrict__ batch, int N) {
    __shared__ __attribute__((aligned(16))) short joined[kPacketRowsPerBlock][2 * 512];      // carry[0:c] ++ packet, < 2N samples
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * kPacketRowsPerBlock + w;
    const bool live = i < n_rows;                // (no early return: the barriers are the workgroup's)
    const int4 e = live ? table[i] : make_int4(0, 0, 0, 0);
    const int b = e.x, off = e.y, len = e.z, c = e.w, at = lane * 8;
    short *row = joined[w];
    i16x8 *crow = reinterpret_cast<i16x8 *>(carry + (size_t)b * N);
    i16x8 v = {};
    if (off >= 0 && at < len) v = __builtin_nontemporal_load(reinterpret_cast<const i16x8 *>(pkt + off) + lane);      // (a silent row: zeros)
    if (at < c) *reinterpret_cast<i16x8 *>(row + at) = crow[lane];
    __syncthreads();
    // the packet behind the pending samples, at the unaligned offset c
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (at + j < len) row[c + at + j] = v[j];
    __syncthreads();
    const int base = c + len >= N ? N : 0, rest = c + len - base;     // base N: a chunk is complete, the rest is the new carry
    if (base && at < N) batch[(size_t)b * (N / 8) + lane] = *reinterpret_cast<const i16x8 *>(row + at);
    if (at < rest) crow[lane] = *reinterpret_cast<const i16x8 *>(row + base + at);
}

// assemble_packets for a tick with G.711 rows: the row table's offsets are in bytes and len carries the row's codec in its high bits
// (uniform across the wave).  An S16 row moves as above; a G.711 row's lane loads 16 codes (16 bytes, N / 16 <= 32 lanes cover a row),
// expands them in registers and writes them into the LDS row at c + 16 * lane.  The carry and batch stores are those of
// assemble_packets: the carry holds expanded int16, whatever format the packets arrived in.
using u32x4 = unsigned __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64 * kPacketRowsPerBlock) assemble_coded_packets_kernel(const int4 *__restrict__ table, long n_rows,
                                                                                           const uint8_t *__restrict__ pkt, int16_t *carry,
                                                                                           i16x8 *__restrict__ batch, int N) {
    __shared__ __attribute__((aligned(16))) short joined[kPacketRowsPerBlock][2 * 512];      // carry[0:c] ++ packet, < 2N samples
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * kPacketRowsPerBlock + w;
    const bool live = i < n_rows;                // (no early return: the barriers are the workgroup's)
    const int4 e = live ? table[i] : make_int4(0, 0, 0, 0);
    const int b = e.x, off = e.y, len = e.z & ((1 << kCodecShift) - 1), codec = e.z >> kCodecShift, c = e.w, at = lane * 8;
    short *row = joined[w];
    i16x8 *crow = reinterpret_cast<i16x8 *>(carry + (size_t)b * N);
    const int from = codec == VAD_PCM_S16 ? at : lane * 16;         // the lane's first sample of the packet: 16 bytes hold 8 or 16
    u32x4 v = {};
    if (off >= 0 && from < len) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(pkt + off) + lane);     // (a silent row: S16 zeros)
    if (at < c) *reinterpret_cast<i16x8 *>(row + at) = crow[lane];
    __syncthreads();
    // the packet behind the pending samples, at the unaligned offset c
    if (codec == VAD_PCM_S16) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (from + j < len) row[c + from + j] = (short)(v[j >> 1] >> (16 * (j & 1)));
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (from + j < len) row[c + from + j] = g711_to_s16(codec, (uint8_t)(v[j >> 2] >> (8 * (j & 3))));
    }
    __syncthreads();
    const int base = c + len >= N ? N : 0, rest = c + len - base;     // base N: a chunk is complete, the rest is the new carry
    if (base && at < N) batch[(size_t)b * (N / 8) + lane] = *reinterpret_cast<const i16x8 *>(row + at);
    if (at < rest) crow[lane] = *reinterpret_cast<const i16x8 *>(row + base + at);
}

// DVI4 (VAD_PCM_DVI4, adpcm.hpp): a row is {predict, index, reserved} and then 4-bit IMA ADPCM codes, and decoding them is a recurrence
// -- (pred, idx) runs from sample to sample.  Both updates are saturating adds, and saturating adds compose (adpcm_then), so a wave
// decodes up to 512 samples with two inclusive scans over that monoid instead of one lane walking the row:
//   lane l holds dword 1 + l of the row = the codes of samples 8 l ... 8 l + 7 (first sample in the high nibble of the first byte);
//   scan 1 over (IDX[d], 0, 88): the lane folds its 8 codes, six __shfl_up rounds scan the folds across the lanes, the fold of the lanes
//     in front applied to the header's index is the lane's first index, and the lane walks its 8 codes from there: 8 steps (the 89-entry
//     table sits in LDS, the lanes index it divergently) and with them 8 signed changes +-v;
//   scan 2 over (+-v, -32768, 32767): the same fold / scan / re-apply from the header's predictor gives the 8 samples.
// Codes behind the row's last sample (a zero register, or the bytes up to the row's 16-byte end) sit behind every sample that is
// stored: an inclusive scan never carries them forward.  Integer arithmetic only, no atomics; the scans need the whole wave, and the
// row's codec is uniform across it.
__device__ inline AdpcmSat wave_scan_before(AdpcmSat f, int lane) {
    // -> the composition of the lanes in FRONT of this one (lane 0: the identity)
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const AdpcmSat g{__shfl_up(f.a, s, 64), __shfl_up(f.lo, s, 64), __shfl_up(f.hi, s, 64)};
        if (lane >= s) f = adpcm_then(g, f);
    }
    const AdpcmSat g{__shfl_up(f.a, 1, 64), __shfl_up(f.lo, 1, 64), __shfl_up(f.hi, 1, 64)};
    return lane ? g : adpcm_identity();
}

// One piece of a DVI4 row: w = the lane's 8 codes, (pred, idx) = the decoder's state in front of the piece's first sample (uniform).
// out[j] <- sample 8 lane + j of the piece; (pred, idx) <- the state behind the lane's last code.
__device__ inline void adpcm_decode_wave(unsigned w, int lane, const short *steps, int &pred, int &idx, int (&out)[8]) {
    unsigned d[8];
    AdpcmSat f = adpcm_identity();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        d[j] = (w >> (8 * (j >> 1) + (j & 1 ? 0 : 4))) & 15u;
        f = adpcm_then(f, AdpcmSat{adpcm_index_add(d[j]), 0, kAdpcmMaxIndex});
    }
    idx = adpcm_apply(wave_scan_before(f, lane), idx);
    f = adpcm_identity();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        out[j] = adpcm_delta(steps[idx], d[j]);
        idx = adpcm_clamp(idx + adpcm_index_add(d[j]), 0, kAdpcmMaxIndex);
        f = adpcm_then(f, AdpcmSat{out[j], -32768, 32767});
    }
    pred = adpcm_apply(wave_scan_before(f, lane), pred);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = pred = adpcm_clamp(pred + out[j], -32768, 32767);
}

// the header dword of a DVI4 row as the little-endian load delivers it -> (predict: big-endian on the wire, index: above 88 used as 88)
__device__ inline void adpcm_header(unsigned h, int &pred, int &idx) {
    pred = adpcm_header_predict(h, h >> 8);
    idx = adpcm_header_index(h >> 16);
}

// assemble_coded_packets for a tick with at least one DVI4 row: the same table, the same LDS splice, the same 16-byte carry and batch
// stores; S16 and G.711 rows move as there.  A DVI4 row's lane loads ONE dword of codes (8 samples: 64 lanes cover N = 512) and every
// lane the header dword; the decoded samples go into the LDS row at c + 8 lane + j.
__global__ void __launch_bounds__(64 * kPacketRowsPerBlock) assemble_adpcm_packets_kernel(const int4 *__restrict__ table, long n_rows,
                                                                                           const uint8_t *__restrict__ pkt, int16_t *carry,
                                                                                           i16x8 *__restrict__ batch, int N) {
    __shared__ __attribute__((aligned(16))) short joined[kPacketRowsPerBlock][2 * 512];      // carry[0:c] ++ packet, < 2N samples
    __shared__ short steps[kAdpcmSteps];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * kPacketRowsPerBlock + w;
    const bool live = i < n_rows;                // (no early return: the barriers are the workgroup's)
    const int4 e = live ? table[i] : make_int4(0, 0, 0, 0);
    const int b = e.x, off = e.y, len = e.z & ((1 << kCodecShift) - 1), codec = e.z >> kCodecShift, c = e.w, at = lane * 8;
    short *row = joined[w];
    i16x8 *crow = reinterpret_cast<i16x8 *>(carry + (size_t)b * N);
    const bool dvi4 = codec == VAD_PCM_DVI4;
    const int from = codec == VAD_PCM_S16 || dvi4 ? at : lane * 16;         // the lane's first sample of the packet
    u32x4 v = {};
    unsigned head = 0;
    if (dvi4) {                                  // (never a silent row: those are S16; dword 1 + lane ends inside the row's 16-byte end)
        const unsigned *src = reinterpret_cast<const unsigned *>(pkt + off);
        head = src[0];
        if (from < len) v[0] = __builtin_nontemporal_load(src + 1 + lane);
    } else if (off >= 0 && from < len)
        v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(pkt + off) + lane);     // (a silent row: S16 zeros)
    if (threadIdx.x < kAdpcmSteps) steps[threadIdx.x] = (short)adpcm_step_of(threadIdx.x);
    if (at < c) *reinterpret_cast<i16x8 *>(row + at) = crow[lane];
    __syncthreads();
    // the packet behind the pending samples, at the unaligned offset c
    if (dvi4) {
        int pred, idx, out[8];
        adpcm_header(head, pred, idx);
        adpcm_decode_wave(v[0], lane, steps, pred, idx, out);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (from + j < len) row[c + from + j] = (short)out[j];
    } else if (codec == VAD_PCM_S16) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (from + j < len) row[c + from + j] = (short)(v[j >> 1] >> (16 * (j & 1)));
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (from + j < len) row[c + from + j] = g711_to_s16(codec, (uint8_t)(v[j >> 2] >> (8 * (j & 3))));
    }
    __syncthreads();
    const int base = c + len >= N ? N : 0, rest = c + len - base;     // base N: a chunk is complete, the rest is the new carry
    if (base && at < N) batch[(size_t)b * (N / 8) + lane] = *reinterpret_cast<const i16x8 *>(row + at);
    if (at < rest) crow[lane] = *reinterpret_cast<const i16x8 *>(row + base + at);
}

// assemble_packets for a wide tick (vad_pump_submit_wide_packets): int16 rows sampled at step x 16 kHz, of which the comb k0, k0 + step,
// ... is kept (device_api.hpp comb_first / comb_kept; step and k0 ride in the high bits of len, uniform across the wave).  Lane l owns
// the input samples [8 step l, 8 step (l + 1)) of its row: `step` consecutive 16-byte loads.  The span starts on a multiple of step, so
// whatever k0 is it holds exactly 8 kept samples and 8 l kept samples lie in front of it: the lane writes them at c + 8 l + j of the
// LDS row without a scan, each guarded by the row's length.  N / 8 lanes cover the longest row (step * N), at most N samples are kept,
// and what follows the second barrier is assemble_packets with `kept` for len.
template <int STEP>
__device__ inline void keep_comb(const i16x8 (&v)[kMaxWideStep], int k0, int left, short *dst) {
#pragma unroll
    for (int q = 0; q < STEP; ++q) {             // (k0 is uniform: one of the STEP bodies runs, its indices are constants)
        if (k0 != q) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (q + STEP * j < left) dst[j] = v[(q + STEP * j) >> 3][(q + STEP * j) & 7];
    }
}

__global__ void __launch_bounds__(64 * kPacketRowsPerBlock) assemble_wide_packets_kernel(const int4 *__restrict__ table, long n_rows,
                                                                                          const uint8_t *__restrict__ pkt, int16_t *carry,
                                                                                          i16x8 *__restrict__ batch, int N) {
    __shared__ __attribute__((aligned(16))) short joined[kPacketRowsPerBlock][2 * 512];      // carry[0:c] ++ kept samples, < 2N samples
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * kPacketRowsPerBlock + w;
    const bool live = i < n_rows;                // (no early return: the barriers are the workgroup's)
    const int4 e = live ? table[i] : make_int4(0, 0, 1 << kCodecShift, 0);
    const int b = e.x, off = e.y, len = e.z & ((1 << kCodecShift) - 1), step = (e.z >> kCodecShift) & 15, k0 = e.z >> kCombShift, c = e.w;
    const int at = lane * 8, from = at * step;   // the lane's first kept sample of the row, its first input sample
    const int kept = comb_kept(step, k0, len);
    short *row = joined[w];
    i16x8 *crow = reinterpret_cast<i16x8 *>(carry + (size_t)b * N);
    const i16x8 *src = reinterpret_cast<const i16x8 *>(pkt + off) + step * lane;     // (a silent row: never dereferenced)
    i16x8 v[kMaxWideStep] = {};
#pragma unroll
    for (int m = 0; m < kMaxWideStep; ++m)
        if (off >= 0 && m < step && from + 8 * m < len) v[m] = __builtin_nontemporal_load(src + m);      // (a silent row: zeros)
    if (at < c) *reinterpret_cast<i16x8 *>(row + at) = crow[lane];
    __syncthreads();
    // the kept samples behind the pending ones, at the unaligned offset c
    if (step == 1) keep_comb<1>(v, k0, len - from, row + c + at);
    else if (step == 2) keep_comb<2>(v, k0, len - from, row + c + at);
    else keep_comb<3>(v, k0, len - from, row + c + at);
    __syncthreads();
    const int base = c + kept >= N ? N : 0, rest = c + kept - base;   // base N: a chunk is complete, the rest is the new carry
    if (base && at < N) batch[(size_t)b * (N / 8) + lane] = *reinterpret_cast<const i16x8 *>(row + at);
    if (at < rest) crow[lane] = *reinterpret_cast<const i16x8 *>(row + base + at);
}

// assemble_burst (burst ticks, vad_pump_submit_burst): several rows per stream, rows longer than N.  The kernels above are one wave
// per ROW and rely on nobody else touching the row's carry; with several rows of one stream in a tick the wave that writes the new carry
// would race the wave that reads the old one.  Here the work unit is the STREAM.  The host grouped the table's rows by stream; the wave
// whose row is the first of its stream walks that stream's rows in order, the waves of its other rows have nothing to do.  One wave is
// one workgroup, so the walk (whose length differs from stream to stream) may use the workgroup barrier.  `joined` holds carry[0:c] ++
// what has arrived since, always < 2N samples: a row goes in in pieces of at most N samples (16-byte loads: 8 samples of int16 or 16
// G.711 codes a lane, expanded in registers, written at the unaligned fill), and whenever N samples are there they leave as one chunk
// (16-byte stores) and the rest moves to the front.  What is left at the end (< N) is the new carry, stored in place.
//
// ADPCM (a tick with at least one DVI4 row; the instantiation without it is the kernel as it always was): a DVI4 row goes in in the same
// pieces of at most N samples, a dword of 8 codes a lane, decoded by adpcm_decode_wave.  The decoder's state in front of the row's
// first piece is the header's; behind a whole piece it is the state behind sample N - 1, lane N / 8 - 1's, broadcast to the wave.
template <bool ADPCM>
__global__ void __launch_bounds__(64) assemble_burst_kernel(const int4 *__restrict__ table, long n_rows, const uint8_t *__restrict__ pkt,
                                                            int16_t *carry, i16x8 *__restrict__ batch, i16x8 *__restrict__ more,
                                                            int max_chunks, long streams, int N) {
    __shared__ __attribute__((aligned(16))) short joined[2 * 512];
    __shared__ short steps[ADPCM ? kAdpcmSteps : 1];
    const int lane = threadIdx.x, at = lane * 8;
    const long i0 = blockIdx.x;
    const int4 first = table[i0];
    if (first.w < 0) return;                     // (uniform: not the first row of its stream)
    const int b = first.x;
    i16x8 *crow = reinterpret_cast<i16x8 *>(carry + (size_t)b * N);
    int fill = first.w & ((1 << kCodecShift) - 1), chunk = 0;
    if (at < fill) *reinterpret_cast<i16x8 *>(joined + at) = crow[lane];
    if constexpr (ADPCM) {
        steps[lane] = (short)adpcm_step_of(lane);
        if (lane + 64 < kAdpcmSteps) steps[lane + 64] = (short)adpcm_step_of(lane + 64);
    }
    __syncthreads();
    for (long i = i0; i < n_rows; ++i) {
        const int4 e = i == i0 ? first : table[i];
        if (i != i0 && (e.x != b || e.w >= 0)) break;                           // the next stream's first row
        const int len = e.z & ((1 << kCodecShift) - 1), codec = e.z >> kCodecShift;
        const int per = codec == VAD_PCM_S16 ? 8 : 16;                         // samples in a lane's 16 bytes
        const bool quiet = e.y < 0;                                             // a silent row: its pieces are zeros, pkt is not touched
        const u32x4 *src = reinterpret_cast<const u32x4 *>(pkt + e.y);                     // (... nor is this)
        const bool dvi4 = ADPCM && codec == VAD_PCM_DVI4;                       // (never a silent row: those are S16)
        int pred = 0, idx = 0;                                                  // a DVI4 row: the decoder's state in front of the piece
        if (dvi4) adpcm_header(*reinterpret_cast<const unsigned *>(src), pred, idx);
        for (int s0 = 0; s0 < len; s0 += N) {                                   // a piece: samples [s0, s0 + n) of the row
            const int n = min(N, len - s0), from = dvi4 ? at : lane * per;
            u32x4 v = {};
            if (dvi4) {                                                         // (dword 1 + s0 / 8 + lane ends inside the row's 16-byte end)
                if (from < n) v[0] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(src) + 1 + s0 / 8 + lane);
            } else if (!quiet && from < n)
                v = __builtin_nontemporal_load(src + s0 / per + lane);
            short *dst = joined + fill + from;
            if (dvi4) {
                int out[8];
                adpcm_decode_wave(v[0], lane, steps, pred, idx, out);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (from + j < n) dst[j] = (short)out[j];
                pred = __shfl(pred, N / 8 - 1, 64);                             // (of use behind a whole piece only)
                idx = __shfl(idx, N / 8 - 1, 64);
            } else if (codec == VAD_PCM_S16) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (from + j < n) dst[j] = (short)(v[j >> 1] >> (16 * (j & 1)));
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (from + j < n) dst[j] = g711_to_s16(codec, (uint8_t)(v[j >> 2] >> (8 * (j & 3))));
            }
            __syncthreads();
            fill += n;
            if (fill < N) continue;
            // a chunk is complete: joined[0:N] leaves, joined[N:fill] moves to the front
            const i16x8 out = *reinterpret_cast<const i16x8 *>(joined + at), rest = *reinterpret_cast<const i16x8 *>(joined + N + at);
            if (at < N && chunk < max_chunks) {
                i16x8 *row = chunk == 0 ? batch + (size_t)b * (N / 8) : more + ((size_t)(chunk - 1) * streams + b) * (N / 8);
                row[lane] = out;
            }
            __syncthreads();
            fill -= N;
            ++chunk;
            if (at < fill) *reinterpret_cast<i16x8 *>(joined + at) = rest;
            __syncthreads();
        }
    }
    if (at < fill) crow[lane] = *reinterpret_cast<const i16x8 *>(joined + at);
}

// assemble_resampled_packets (resampled packet ticks, vad_pump_submit_resampled_packets): int16 rows at 44.1 / 24 / 22.05 / ... kHz pass
// the polyphase filter of kernel_resample.hip on their way into the stream's chunk -- the STREAMING form of that filter: a stream keeps
// the last H = K - 1 input samples (hist, int16) and the outputs that do not fill a chunk yet (carry, fp32), and a row emits exactly the
// outputs whose K inputs have all arrived.  One wave = one workgroup per row (the row's length, and with it the rounds of every loop,
// differ from row to row; the barriers are the wave's own).  The host computed every index (device_api.hpp has the table): the wave
//   1. stages hist[b] ++ row as floats in LDS (int16 / 32768 is exact; a silent row: zeros) and the fp32 carry behind them;
//   2. makes the row's outputs, lane l the outputs l, l + 64, ...: acc = 0.0f; acc = fmaf(taps[k][j], in[k], acc), k = 0 ... K - 1 -- the
//      expression and the tap order of resample_rows_kernel over the same transposed table, so every output carries the bits the batch
//      kernel gives for the concatenated stream (consecutive lanes, consecutive phases: the tap loads are consecutive floats);
//   3. writes the last H staged samples back as the new history (every lane read the old one in front of the first barrier);
//   4. splices carry ++ outputs: if they reach `chunk` the first `chunk` go to the stream's fp32 batch row, the rest is the new carry.
// All LDS is dynamic and moves as 32-bit words: in[hist_ld + max_len] ++ joined[2 chunk].  No atomics; nobody else touches the row's
// history, carry or batch row (one row per stream and tick).
constexpr int kResampleOutputsInFlight = 4;

__global__ void __launch_bounds__(64) assemble_resampled_packets_kernel(const int4 *__restrict__ table, const uint8_t *__restrict__ pkt,
                                                                        PumpRates R, int16_t *hist, int hist_ld, int max_len, float *carry,
                                                                        float *__restrict__ batch, int chunk) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *in = lds, *joined = lds + hist_ld + max_len;
    const int lane = threadIdx.x;
    const int4 e0 = table[2 * (size_t)blockIdx.x], e1 = table[2 * (size_t)blockIdx.x + 1];
    const int b = e0.x, off = e0.y, len = e0.z & ((1 << kResampleRateShift) - 1), r = e0.z >> kResampleRateShift, c = e0.w;
    const int base = e1.x, j0 = e1.y, n_out = e1.z;
    const int O = R.O[r], N = R.N[r], K = R.K[r], H = R.H[r];
    const float *taps = R.taps[r];
    const int32_t *first = R.first[r];
    int16_t *hrow = hist + (size_t)b * hist_ld;
    float *crow = carry + (size_t)b * chunk;
    for (int s = lane; s < H; s += 64) in[s] = (float)hrow[s] * (1.0f / 32768.0f);
    const i16x8 *src = reinterpret_cast<const i16x8 *>(pkt + off);              // (a silent row: never dereferenced)
    for (int at = lane * 8; at < len; at += 64 * 8) {
        i16x8 v = {};
        if (off >= 0) v = __builtin_nontemporal_load(src + at / 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (at + j < len) in[H + at + j] = (float)v[j] * (1.0f / 32768.0f);
    }
    for (int s = lane; s < c; s += 64) joined[s] = crow[s];
    __syncthreads();
    // (kResampleOutputsInFlight outputs of a lane are made side by side -- each its own chain in tap order --: one wave is the whole
    // workgroup, and the tap loads' latency is hidden by the lane's other chains, not by other waves; a slot behind the row's last output
    // recomputes that output and is not stored)
    for (int i0 = lane; i0 < n_out; i0 += 64 * kResampleOutputsInFlight) {
        const float *x[kResampleOutputsInFlight], *h[kResampleOutputsInFlight];
        float acc[kResampleOutputsInFlight];
#pragma unroll
        for (int u = 0; u < kResampleOutputsInFlight; ++u) {
            const int t = j0 + min(i0 + 64 * u, n_out - 1), dq = t / N, j = t - dq * N;
            x[u] = in + (base + dq * O + first[j]);
            h[u] = taps + j;
            acc[u] = 0.0f;
        }
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int u = 0; u < kResampleOutputsInFlight; ++u) acc[u] = fmaf(h[u][(long)k * N], x[u][k], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < kResampleOutputsInFlight; ++u)
            if (i0 + 64 * u < n_out) joined[c + i0 + 64 * u] = acc[u];
    }
    for (int s = lane; s < H; s += 64) hrow[s] = (int16_t)(in[len + s] * 32768.0f);     // (exact: the staged values are n / 32768)
    __syncthreads();
    const int total = c + n_out, done = total >= chunk ? chunk : 0;           // done == chunk: a chunk is complete, the rest is the new carry
    if (done)
        for (int s = lane; s < chunk; s += 64) batch[(size_t)b * chunk + s] = joined[s];
    for (int s = (done ? 0 : c) + lane; s < total - done; s += 64) crow[s] = joined[done + s];
}

// one thread per (sub-step j >= 1, stream): flags[j - 1][b] = k[b] > j
__global__ void __launch_bounds__(256) burst_flags_kernel(const uint8_t *__restrict__ k_of_stream, uint8_t *__restrict__ flags, long ld, int streams) {
    const int b = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y + 1;
    if (b < streams) flags[(size_t)(j - 1) * ld + b] = k_of_stream[b] > j;
}

}  // namespace

hipError_t launch_assemble_burst(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int16_t *more,
                                 int max_chunks, int streams, int N, bool adpcm, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!table || !pkt || !carry || !batch || (max_chunks > 1 && !more) || max_chunks < 1 || streams <= 0 || N <= 0 || N > 512 || N % 16)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(adpcm ? assemble_burst_kernel<true> : assemble_burst_kernel<false>, dim3((unsigned)n_rows), dim3(64), 0, s,
                       reinterpret_cast<const int4 *>(table), n_rows, pkt, carry, reinterpret_cast<i16x8 *>(batch),
                       reinterpret_cast<i16x8 *>(more), max_chunks, (long)streams, N);
    return hipGetLastError();
}

hipError_t launch_burst_flags(const uint8_t *k_of_stream, uint8_t *flags, long ld, int steps, int streams, hipStream_t s) {
    if (steps <= 1 || streams <= 0) return hipSuccess;
    if (!k_of_stream || !flags || ld < streams) return hipErrorInvalidValue;
    hipLaunchKernelGGL(burst_flags_kernel, dim3((unsigned)((streams + 255) / 256), (unsigned)(steps - 1)), dim3(256), 0, s, k_of_stream, flags, ld,
                       streams);
    return hipGetLastError();
}

hipError_t launch_assemble_packets(const int32_t *table, long n_rows, const int16_t *pkt, int16_t *carry, int16_t *batch, int N, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!table || !pkt || !carry || !batch || N <= 0 || N > 512 || N % 8) return hipErrorInvalidValue;
    const long blocks = (n_rows + kPacketRowsPerBlock - 1) / kPacketRowsPerBlock;
    hipLaunchKernelGGL(assemble_packets_kernel, dim3((unsigned)blocks), dim3(64 * kPacketRowsPerBlock), 0, s,
                       reinterpret_cast<const int4 *>(table), n_rows, pkt, carry, reinterpret_cast<i16x8 *>(batch), N);
    return hipGetLastError();
}

hipError_t launch_assemble_coded_packets(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int N,
                                         hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!table || !pkt || !carry || !batch || N <= 0 || N > 512 || N % 8) return hipErrorInvalidValue;
    const long blocks = (n_rows + kPacketRowsPerBlock - 1) / kPacketRowsPerBlock;
    hipLaunchKernelGGL(assemble_coded_packets_kernel, dim3((unsigned)blocks), dim3(64 * kPacketRowsPerBlock), 0, s,
                       reinterpret_cast<const int4 *>(table), n_rows, pkt, carry, reinterpret_cast<i16x8 *>(batch), N);
    return hipGetLastError();
}

hipError_t launch_assemble_adpcm_packets(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int N,
                                         hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!table || !pkt || !carry || !batch || N <= 0 || N > 512 || N % 8) return hipErrorInvalidValue;
    const long blocks = (n_rows + kPacketRowsPerBlock - 1) / kPacketRowsPerBlock;
    hipLaunchKernelGGL(assemble_adpcm_packets_kernel, dim3((unsigned)blocks), dim3(64 * kPacketRowsPerBlock), 0, s,
                       reinterpret_cast<const int4 *>(table), n_rows, pkt, carry, reinterpret_cast<i16x8 *>(batch), N);
    return hipGetLastError();
}

hipError_t launch_assemble_wide_packets(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int N,
                                        hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    if (!table || !pkt || !carry || !batch || N <= 0 || N > 512 || N % 8) return hipErrorInvalidValue;
    const long blocks = (n_rows + kPacketRowsPerBlock - 1) / kPacketRowsPerBlock;
    hipLaunchKernelGGL(assemble_wide_packets_kernel, dim3((unsigned)blocks), dim3(64 * kPacketRowsPerBlock), 0, s,
                       reinterpret_cast<const int4 *>(table), n_rows, pkt, carry, reinterpret_cast<i16x8 *>(batch), N);
    return hipGetLastError();
}

hipError_t launch_assemble_resampled_packets(const int32_t *table, long n_rows, const uint8_t *pkt, const PumpRates &rates, int16_t *hist,
                                             int hist_ld, int max_len, float *carry, float *batch, int chunk, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const size_t lds = ((size_t)hist_ld + (size_t)max_len + 2 * (size_t)chunk) * sizeof(float);
    if (!table || !pkt || !hist || !carry || !batch || chunk <= 0 || hist_ld <= 0 || hist_ld % 4 || max_len <= 0 || max_len % 8 || lds > 65536 ||
        n_rows > 0x7fffffffL)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(assemble_resampled_packets_kernel, dim3((unsigned)n_rows), dim3(64), lds, s, reinterpret_cast<const int4 *>(table), pkt,
                       rates, hist, hist_ld, max_len, carry, batch, chunk);
    return hipGetLastError();
}

hipError_t launch_expand_rows(const uint8_t *present, const int32_t *pos, const uint8_t *src, void *dst, long row_bytes, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!present || !pos || row_bytes <= 0 || row_bytes % 16) return hipErrorInvalidValue;
    const int vec = (int)(row_bytes / 16);
    const long threads = (long)B * vec;
    hipLaunchKernelGGL(expand_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, present, pos,
                       reinterpret_cast<const f32x4 *>(src), static_cast<f32x4 *>(dst), vec, B);
    return hipGetLastError();
}

hipError_t launch_carry_absent(const uint8_t *present, const float *ctx_in, float *ctx_out, int C, float *probs, long ldp, int B,
                               hipStream_t s) {
    if (B <= 0 || !present) return hipSuccess;
    const int vec = C / 4;
    const long threads = (long)B * vec;
    hipLaunchKernelGGL(carry_absent_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, present, ctx_in, ctx_out, vec, probs, ldp, B);
    return hipGetLastError();
}

}  // namespace vad
