// kernel_tape.hip -- the pump's TAPE: every live stream's recent net-rate int16 audio in HBM, and any still-held sample range of any set
// of streams copied out of it, packed (include/silero_vad_hip.h "THE TAPE"; the window rule and the ring's addressing are tape.hpp).
//
// What a consumer of the pump's events wants next is the audio between a START and an END: the reference's flow is VADIterator events,
// then the slice audio[start:end] (examples/microphone_and_webRTC_integration; collect_chunks, src/silero_vad/utils_vad.py:552-590).  On
// the packet routes the host never has that audio -- G.711 rows are expanded, 32 / 48 kHz rows combed, silent rows spliced in on the
// device -- but every route ends in the same batch rows the step kernels read, so the tape is written there.
//
//   * TAPE (tape_rows_kernel, once per step of a tick, on the compute stream behind the step's last part): stream b, if its flag is set
//     (or the step has no flags), copies its batch row into ring slot count[b] % chunks of its tape and adds 1 to count[b]; a stream
//     whose flag is 0 is untouched, exactly like its (h, c).  A row is N / 8 lanes of one 16-byte load and store (64 lanes at N = 512,
//     32 at N = 256: a row never spans two waves, so the lanes' reads of the counter precede lane 0's write of it in program order);
//     256 threads = 4 / 8 rows per workgroup, one workgroup per 4 / 8 streams: HBM to HBM, as wide as the batch.  The counter is
//     written with an ordinary vector store from the row's first lane.
//   * GATHER (tape_gather_kernel): work is dealt by OUTPUT tile, like collect_segments_kernel.  A grid of one-wave workgroups walks the
//     (request, 8 KiB output tile) pairs; a tile behind the request's last sample is left at once.  A request is one run of at most
//     chunks * N samples of one stream's clock, so it wraps the ring at most once: element e0 = first % (chunks * N) is computed once per
//     item, a lane's element is e0 + its output index, less the ring's length where it passes it.
//       fast path  the lane's 16 output bytes come from one side of the wrap, all 8 samples are wanted and the destination is 16-byte
//                  aligned: the source starts at ANY sample, so the lane reads the aligned granule that holds its first byte and, where
//                  that byte is not the granule's first, the next one -- a granule that holds a wanted byte lies in the stream's ring, so
//                  no load reaches past the last stream's last chunk -- and funnels the 16 bytes out of the pair (v_alignbyte, as
//                  kernel_collect.hip); one aligned 16-byte store.  The 8 vectors' loads are issued before the first store.
//       slow path  a lane that straddles the wrap, a request's last partial vector, a destination that is not 16-byte aligned: element
//                  by element (a 2-byte store costs ~12 x a 16-byte store per byte on this part: that is why it is the exception).
//     Exactly count samples are written per request; padding between requests is never touched.
#include <hip/hip_runtime.h>

#include "device_api.hpp"
#include "tape.hpp"

namespace vad {
namespace {

constexpr int kTapeBlock = 256;                    // threads of a tape_rows workgroup
constexpr int kTileBytes = 8192;                   // one wave-iteration of the gather: 64 lanes x 16 B x 8
constexpr long kTileElems = kTileBytes / 2;
using u32x4 = unsigned __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(kTapeBlock) tape_rows_kernel(const int16_t *rows, const uint8_t *flags, int16_t *tape, int64_t *clock,
                                                                int chunks, int streams, int N) {
    const int lanes = N >> 3;                      // lanes of a row: 16 bytes each
    const int b = blockIdx.x * (kTapeBlock / lanes) + (int)threadIdx.x / lanes, l = (int)threadIdx.x % lanes;
    if (b >= streams) return;
    if (flags && !flags[b]) return;
    const int64_t c = clock[2 * (size_t)b];
    const size_t at = ((size_t)b * chunks + (size_t)tape_slot(c, chunks)) * N + (size_t)l * 8;
    *reinterpret_cast<u32x4 *>(tape + at) = *reinterpret_cast<const u32x4 *>(rows + (size_t)b * N + (size_t)l * 8);
    if (l == 0) clock[2 * (size_t)b] = c + 1;
}

// bytes [m, m + 16) of the 32 bytes c ++ n; m differs from lane to lane (kernel_collect.hip)
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

__global__ void __launch_bounds__(64) tape_gather_kernel(const TapeRequest *req, long n_req, long tiles_per_req, const int16_t *tape,
                                                         int chunks, int N, int16_t *out) {
    const int lane = threadIdx.x;
    const long items = n_req * tiles_per_req;
    const long ring = (long)chunks * N;            // elements of a stream's ring
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        // everything up to the vectors is wave-uniform
        const long r = item / tiles_per_req, tile = item % tiles_per_req;
        const TapeRequest q = req[r];
        const long want = (long)q.count;           // (the host has confined it to the window: 0 ... ring)
        if (tile * kTileElems >= want) continue;
        const long e0 = (long)tape_element(q.first, chunks, N);
        const uint16_t *src = reinterpret_cast<const uint16_t *>(tape) + (size_t)q.stream * ring;
        uint16_t *dst = reinterpret_cast<uint16_t *>(out) + q.out_offset;
        const bool vec_dst = (((size_t)dst) & 15) == 0;
        long o0[8];
        int mode[8];                               // 0: nothing, 1: fast, 2: slow
        const uint16_t *sp[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            o0[v] = tile * kTileElems + (long)(v * 64 + lane) * 8;
            mode[v] = 0, sp[v] = nullptr;
            if (o0[v] >= want) continue;
            long e = e0 + o0[v];                   // (o0 < want <= ring: the run passes the ring's end at most once)
            const bool before = e + 8 <= ring;     // the lane's 8 samples end in front of the wrap ...
            if (e >= ring) e -= ring;              // ... or start behind it
            if (vec_dst && o0[v] + 8 <= want && (before || e0 + o0[v] >= ring)) {
                sp[v] = src + e;
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
                *reinterpret_cast<u32x4 *>(dst + o0[v]) = funnel(c[v], nx[v], (int)(((size_t)sp[v]) & 15));
            } else if (mode[v] == 2) {
                unsigned w[4] = {0u, 0u, 0u, 0u};
                int got = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long o = o0[v] + j;
                    if (o >= want) continue;
                    long e = e0 + o;
                    if (e >= ring) e -= ring;
                    w[j >> 1] |= (unsigned)src[e] << (16 * (j & 1));
                    got = j + 1;
                }
                if (got == 8 && vec_dst) {
                    *reinterpret_cast<u32x4 *>(dst + o0[v]) = u32x4{w[0], w[1], w[2], w[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (j >= got) continue;
                        dst[o0[v] + j] = (uint16_t)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
                    }
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_tape_rows(const int16_t *rows, const uint8_t *flags, int16_t *tape, int64_t *clock, int chunks, int streams, int N,
                            hipStream_t s) {
    if (streams <= 0) return hipSuccess;
    const int lanes = N / 8;                       // a row is whole 16-byte vectors and lies inside one wave
    if (N % 8 || lanes < 1 || lanes > 64 || 64 % lanes || chunks < 1) return hipErrorInvalidValue;
    const int rows_per_block = kTapeBlock / lanes;
    hipLaunchKernelGGL(tape_rows_kernel, dim3((unsigned)((streams + rows_per_block - 1) / rows_per_block)), dim3(kTapeBlock), 0, s, rows, flags,
                       tape, clock, chunks, streams, N);
    return hipGetLastError();
}

hipError_t launch_tape_gather(const TapeRequest *req, long n_req, long max_count, const int16_t *tape, int chunks, int N, int16_t *out,
                              hipStream_t s) {
    if (n_req <= 0 || max_count <= 0) return hipSuccess;
    if (max_count > (long)chunks * N) return hipErrorInvalidValue;
    const long tiles = (max_count + kTileElems - 1) / kTileElems;
    const long items = n_req * tiles;
    if (items > 0x7fffffffL) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(items < 4096 ? items : 4096);   // HBM to HBM: as wide as the chip (launch_collect_segments)
    hipLaunchKernelGGL(tape_gather_kernel, dim3(grid), dim3(64), 0, s, req, n_req, tiles, tape, chunks, N, out);
    return hipGetLastError();
}

}  // namespace vad
