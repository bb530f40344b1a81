// kernel_tape.hip -- the pump's TAPE: every live stream's recent net-rate audio in HBM, int16 or float32, and any still-held sample range
// of any set of streams copied out of it, packed (include/silero_vad_hip.h "THE TAPE"; the window rule and the ring's addressing are
// tape.hpp).
//
// What a consumer of the pump's events wants next is the audio between a START and an END: the reference's flow is VADIterator events,
// then the slice audio[start:end] (examples/microphone_and_webRTC_integration; collect_chunks, src/silero_vad/utils_vad.py:552-590).  On
// the packet routes the host never has that audio -- G.711 rows are expanded, 32 / 48 kHz rows combed, silent rows spliced in, 44.1 kHz
// rows filtered to fp32 on the device -- but every route ends in the same batch rows the step kernels read, so the tape is written there.
//
//   * TAPE (tape_rows_kernel, once per step of a tick, on the compute stream behind the step's last part): stream b, if its flag is set
//     (or the step has no flags), copies its batch row into ring slot count[b] % chunks of its tape and adds 1 to count[b]; a stream
//     whose flag is 0 is untouched, exactly like its (h, c).  A row is N / 8 lanes of 8 samples, whatever the element (64 lanes at
//     N = 512, 32 at N = 256: a row never spans two waves, so the lanes' reads of the counter precede lane 0's write of it in program
//     order -- a float row of 16 bytes a lane would be 128 lanes, two waves, and the second might read the counter the first has
//     advanced); 256 threads = 4 / 8 rows per workgroup, one workgroup per 4 / 8 streams: HBM to HBM, as wide as the batch.  The counter
//     is written with an ordinary vector store from the row's first lane.  Three forms, by source and destination element:
//       int16 -> int16  one 16-byte load and store a lane.
//       int16 -> float  the one 16-byte load; the lane's 8 samples become (float)x * (1.0f / 32768.0f) (load_pcm, exact) and leave in two
//                       16-byte stores ADJACENT to each other, floats 8 l ... 8 l + 7: they are the lane's own samples, any other
//                       placement would move values between lanes.  The two store instructions of a wave interleave in 16-byte pieces
//                       and together fill whole 32-byte runs a lane, whole cache lines a pair of lanes.
//       float -> float  two 16-byte loads and stores a lane, `lanes` vectors APART: vector v of lane l is floats 4 (v lanes + l) ...,
//                       so each instruction of the wave covers one contiguous half of the row (1 KiB at N = 512), the coalesced
//                       shape; nothing ties a lane to particular samples of a plain copy.
//   * GATHER (tape_gather_kernel): work is dealt by OUTPUT tile, like collect_segments_kernel.  A grid of one-wave workgroups walks the
//     (request, 8 KiB output tile) pairs; a tile behind the request's last sample is left at once.  A request is one run of at most
//     chunks * N samples of one stream's clock, so it wraps the ring at most once: element e0 = first % (chunks * N) is computed once per
//     item, a lane's element is e0 + its output index, less the ring's length where it passes it.  A lane-vector is 16 bytes: 8 int16
//     samples or 4 floats; a tile is 4096 / 2048 samples.
//       fast path  the lane's 16 output bytes come from one side of the wrap, all its samples are wanted and the destination is 16-byte
//                  aligned: the source starts at ANY sample, so the lane reads the aligned granule that holds its first byte and, where
//                  that byte is not the granule's first, the next one, and funnels the 16 bytes out of the pair (int16: v_alignbyte,
//                  as kernel_collect.hip; float: the misalignment is a whole number of dwords, 0 ... 3, so the dword selects alone);
//                  one aligned 16-byte store.  No load reaches past the ring: a stream's ring starts and ends 16-byte aligned (the
//                  allocation is, and N % 8 == 0 makes chunks * N elements of 2 or 4 bytes a multiple of 16), so an aligned granule that
//                  holds a wanted byte lies wholly inside the stream's ring, and the second granule is read only where the lane's last
//                  byte lies in it.  The 8 vectors' loads are issued before the first store.
//       slow path  a lane that straddles the wrap, a request's last partial vector, a destination that is not 16-byte aligned: element
//                  by element (a 2-byte store costs ~12 x a 16-byte store per byte on this part: that is why it is the exception).
//     Exactly count samples are written per request; padding between requests is never touched.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_api.hpp"
#include "tape.hpp"

namespace vad {
namespace {

constexpr int kTapeBlock = 256;                    // threads of a tape_rows workgroup
constexpr int kTileBytes = 8192;                   // one wave-iteration of the gather: 64 lanes x 16 B x 8
using u32x4 = unsigned __attribute__((ext_vector_type(4)));
using i16x8 = short __attribute__((ext_vector_type(8)));
using f32x4 = float __attribute__((ext_vector_type(4)));

template <typename SrcT, typename DstT>
__global__ void __launch_bounds__(kTapeBlock) tape_rows_kernel(const SrcT *rows, const uint8_t *flags, DstT *tape, int64_t *clock, int chunks,
                                                                int streams, int N) {
    const int lanes = N >> 3;                      // lanes of a row: 8 samples each
    const int b = blockIdx.x * (kTapeBlock / lanes) + (int)threadIdx.x / lanes, l = (int)threadIdx.x % lanes;
    if (b >= streams) return;
    if (flags && !flags[b]) return;
    const int64_t c = clock[2 * (size_t)b];
    const size_t slot = ((size_t)b * chunks + (size_t)tape_slot(c, chunks)) * N, row = (size_t)b * N;
    if constexpr (std::is_same<SrcT, int16_t>::value && std::is_same<DstT, int16_t>::value) {
        *reinterpret_cast<u32x4 *>(tape + slot + (size_t)l * 8) = *reinterpret_cast<const u32x4 *>(rows + row + (size_t)l * 8);
    } else if constexpr (std::is_same<SrcT, int16_t>::value) {
        const i16x8 x = *reinterpret_cast<const i16x8 *>(rows + row + (size_t)l * 8);
        constexpr float k = 1.0f / 32768.0f;       // (load_pcm of device_api.hpp)
        f32x4 *to = reinterpret_cast<f32x4 *>(tape + slot + (size_t)l * 8);
        to[0] = f32x4{(float)x[0] * k, (float)x[1] * k, (float)x[2] * k, (float)x[3] * k};
        to[1] = f32x4{(float)x[4] * k, (float)x[5] * k, (float)x[6] * k, (float)x[7] * k};
    } else {
        const size_t a0 = (size_t)l * 4, a1 = (size_t)(lanes + l) * 4;
        const u32x4 v0 = *reinterpret_cast<const u32x4 *>(rows + row + a0), v1 = *reinterpret_cast<const u32x4 *>(rows + row + a1);
        *reinterpret_cast<u32x4 *>(tape + slot + a0) = v0;
        *reinterpret_cast<u32x4 *>(tape + slot + a1) = v1;
    }
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

// the same where m is a multiple of 4 (a float tape): dwords [m / 4, m / 4 + 4) of the 8 dwords c ++ n
__device__ __forceinline__ u32x4 funnel_dwords(u32x4 c, u32x4 n, int m) {
    const int dq = m >> 2;
    return u32x4{dq == 0 ? c.x : dq == 1 ? c.y : dq == 2 ? c.z : c.w, dq == 0 ? c.y : dq == 1 ? c.z : dq == 2 ? c.w : n.x,
                 dq == 0 ? c.z : dq == 1 ? c.w : dq == 2 ? n.x : n.y, dq == 0 ? c.w : dq == 1 ? n.x : dq == 2 ? n.y : n.z};
}

// T: the tape's element as bits, uint16_t (the int16 tape) or uint32_t (the fp32 tape)
template <typename T>
__global__ void __launch_bounds__(64) tape_gather_kernel(const TapeRequest *req, long n_req, long tiles_per_req, const T *tape, int chunks, int N,
                                                         T *out) {
    constexpr int EV = 16 / (int)sizeof(T);        // elements of a lane-vector: 8 / 4
    constexpr long kTileElems = kTileBytes / (long)sizeof(T);
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
        const T *src = tape + (size_t)q.stream * ring;
        T *dst = out + q.out_offset;
        const bool vec_dst = (((size_t)dst) & 15) == 0;
        long o0[8];
        int mode[8];                               // 0: nothing, 1: fast, 2: slow
        const T *sp[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            o0[v] = tile * kTileElems + (long)(v * 64 + lane) * EV;
            mode[v] = 0, sp[v] = nullptr;
            if (o0[v] >= want) continue;
            long e = e0 + o0[v];                   // (o0 < want <= ring: the run passes the ring's end at most once)
            const bool before = e + EV <= ring;    // the lane's samples end in front of the wrap ...
            if (e >= ring) e -= ring;              // ... or start behind it
            if (vec_dst && o0[v] + EV <= want && (before || e0 + o0[v] >= ring)) {
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
                const int m = (int)(((size_t)sp[v]) & 15);
                if constexpr (sizeof(T) == 2)
                    *reinterpret_cast<u32x4 *>(dst + o0[v]) = funnel(c[v], nx[v], m);
                else
                    *reinterpret_cast<u32x4 *>(dst + o0[v]) = funnel_dwords(c[v], nx[v], m);
            } else if (mode[v] == 2) {
                unsigned w[4] = {0u, 0u, 0u, 0u};
                int got = 0;
#pragma unroll
                for (int j = 0; j < EV; ++j) {
                    const long o = o0[v] + j;
                    if (o >= want) continue;
                    long e = e0 + o;
                    if (e >= ring) e -= ring;
                    if constexpr (sizeof(T) == 2)
                        w[j >> 1] |= (unsigned)src[e] << (16 * (j & 1));
                    else
                        w[j] = src[e];
                    got = j + 1;
                }
                if (got == EV && vec_dst) {
                    *reinterpret_cast<u32x4 *>(dst + o0[v]) = u32x4{w[0], w[1], w[2], w[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < EV; ++j) {
                        if (j >= got) continue;
                        if constexpr (sizeof(T) == 2)
                            dst[o0[v] + j] = (T)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
                        else
                            dst[o0[v] + j] = w[j];
                    }
                }
            }
        }
    }
}

template <typename SrcT, typename DstT>
hipError_t tape_rows(const SrcT *rows, const uint8_t *flags, DstT *tape, int64_t *clock, int chunks, int streams, int N, hipStream_t s) {
    if (streams <= 0) return hipSuccess;
    const int lanes = N / 8;                       // a row is N / 8 lanes of whole 16-byte vectors and lies inside one wave
    if (N % 8 || lanes < 1 || lanes > 64 || 64 % lanes || chunks < 1) return hipErrorInvalidValue;
    const int rows_per_block = kTapeBlock / lanes;
    hipLaunchKernelGGL((tape_rows_kernel<SrcT, DstT>), dim3((unsigned)((streams + rows_per_block - 1) / rows_per_block)), dim3(kTapeBlock), 0, s,
                       rows, flags, tape, clock, chunks, streams, N);
    return hipGetLastError();
}

template <typename T>
hipError_t tape_gather(const TapeRequest *req, long n_req, long max_count, const T *tape, int chunks, int N, T *out, hipStream_t s) {
    if (n_req <= 0 || max_count <= 0) return hipSuccess;
    if (max_count > (long)chunks * N || N % 8) return hipErrorInvalidValue;
    constexpr long kTileElems = kTileBytes / (long)sizeof(T);
    const long tiles = (max_count + kTileElems - 1) / kTileElems;
    const long items = n_req * tiles;
    if (items > 0x7fffffffL) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(items < 4096 ? items : 4096);   // HBM to HBM: as wide as the chip (launch_collect_segments)
    hipLaunchKernelGGL((tape_gather_kernel<T>), dim3(grid), dim3(64), 0, s, req, n_req, tiles, tape, chunks, N, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tape_rows(const int16_t *rows, const uint8_t *flags, int16_t *tape, int64_t *clock, int chunks, int streams, int N,
                            hipStream_t s) {
    return tape_rows(rows, flags, tape, clock, chunks, streams, N, s);
}

hipError_t launch_tape_rows(const int16_t *rows, const uint8_t *flags, float *tape, int64_t *clock, int chunks, int streams, int N,
                            hipStream_t s) {
    return tape_rows(rows, flags, tape, clock, chunks, streams, N, s);
}

hipError_t launch_tape_rows(const float *rows, const uint8_t *flags, float *tape, int64_t *clock, int chunks, int streams, int N, hipStream_t s) {
    return tape_rows(rows, flags, tape, clock, chunks, streams, N, s);
}

hipError_t launch_tape_gather(const TapeRequest *req, long n_req, long max_count, const int16_t *tape, int chunks, int N, int16_t *out,
                              hipStream_t s) {
    return tape_gather(req, n_req, max_count, reinterpret_cast<const uint16_t *>(tape), chunks, N, reinterpret_cast<uint16_t *>(out), s);
}

hipError_t launch_tape_gather(const TapeRequest *req, long n_req, long max_count, const float *tape, int chunks, int N, float *out,
                              hipStream_t s) {
    return tape_gather(req, n_req, max_count, reinterpret_cast<const uint32_t *>(tape), chunks, N, reinterpret_cast<uint32_t *>(out), s);
}

}  // namespace vad
