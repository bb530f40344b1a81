// kernel_ingest.hip -- ragged recordings from PINNED host memory straight into a zero-padded [n][width] batch in HBM.
//
// A corpus run (BASELINE config 4; the reference fans one Python process out per file, examples/parallel_example.ipynb
// cells 5, 7, and pads each file's last chunk with zeros, src/silero_vad/utils_vad.py:326-327) is bounded by the host
// link, and the host side of the staged path (vad_stage_rows: every sample copied once more, pageable RAM -> pinned
// staging, by CPU threads the container has few of) was its second-largest cost in round 2.  When the recordings already
// sit in page-locked memory -- a decoder that writes into hipHostMalloc'ed / hipHostRegister'ed buffers -- nothing needs
// to touch them on the CPU: this kernel reads them over PCIe (host memory is mapped into the GPU's address space) and
// writes the device batch, padding included, in ONE launch for any number of rows.
//
//   * a persistent grid of VAD_GATHER_WAVES (96) ONE-WAVE workgroups walks the (row, 8 KiB segment) pairs, 8 x 16 B per lane in
//     flight: enough outstanding reads for the link, on 9 % of the chip's SIMDs (see the kernel's comment for why so few);
//   * rows whose source address is 16-byte aligned move as 16-byte vectors; others (a view that starts at an odd sample)
//     fall back to element-wise loads for that row (wave-uniform choice) -- correct for any alignment, fast for the usual;
//   * the row table (pointer, length) is itself read from pinned memory, so the host only fills a small table and launches.
#include <hip/hip_runtime.h>

#include "device_api.hpp"

namespace vad {
namespace {

constexpr int kSegBytes = 8192;        // one wave-iteration: 64 lanes x 16 B x 8 loads in flight
#ifndef VAD_GATHER_WAVES
#define VAD_GATHER_WAVES 96
#endif
constexpr int kGatherWaves = VAD_GATHER_WAVES;   // one-wave workgroups: the whole kernel occupies this many of the chip's 1024 SIMDs

// One wave per workgroup, a persistent grid of kGatherWaves: each iteration a wave moves one 8 KiB segment of one row with 8
// independent 16-byte loads per lane in flight (96 waves x 8 KiB = 768 KiB outstanding against PCIe's ~100-150 KB
// bandwidth-delay product; 48 waves reach the same rate alone and lose more to the compute kernels beside them).  The footprint is deliberate: a first version with 256 four-wave workgroups reached the same
// 53 GB/s but sat on every SIMD of the chip, where its registers kept the frontend (two 243-VGPR waves per SIMD) from
// placing its second wave: the compute kernels beside it ran 4x slower (tools/ingest_diag.py).  96 single waves touch 9 % of
// the SIMDs.
__global__ void __launch_bounds__(64) gather_rows_kernel(const RowDesc *rows, long n, long width_bytes, int esz, uint8_t *dst,
                                                         long segs_per_row) {
    using u32x4 = unsigned __attribute__((ext_vector_type(4)));
    const long items = n * segs_per_row;
    const int lane = threadIdx.x;
    __builtin_amdgcn_s_setprio(3);          // few instructions, long waits: let them issue ahead of the compute waves' streams
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long row = item / segs_per_row, seg = item % segs_per_row;
        const uint8_t *src = reinterpret_cast<const uint8_t *>(rows[row].ptr);
        const long live = rows[row].len * esz;                     // bytes that exist; the rest of the row is zero
        uint8_t *d = dst + row * width_bytes;
        const long lo = seg * kSegBytes, hi = lo + kSegBytes < width_bytes ? lo + kSegBytes : width_bytes;
        if ((((size_t)src) & 15) == 0 && lo + kSegBytes <= live && hi == lo + kSegBytes) {
            // the common case: a whole segment inside the recording, 16-byte aligned source -- 8 loads, then 8 stores
            u32x4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src + lo + (k * 64 + lane) * 16L));
#pragma unroll
            for (int k = 0; k < 8; ++k) __builtin_nontemporal_store(v[k], reinterpret_cast<u32x4 *>(d + lo + (k * 64 + lane) * 16L));
        } else if ((((size_t)src) & 15) == 0) {
            // a segment that holds the end of the recording (or of the row): 16-byte vectors, the straddling one byte-wise
            for (long o = lo + lane * 16L; o < hi; o += 64 * 16L) {
                u32x4 v{0u, 0u, 0u, 0u};
                if (o + 16 <= live) {
                    v = *reinterpret_cast<const u32x4 *>(src + o);
                } else if (o < live) {
                    unsigned w[4] = {0u, 0u, 0u, 0u};
                    for (int k = 0; k < (int)(live - o); ++k) w[k >> 2] |= (unsigned)src[o + k] << (8 * (k & 3));
                    v = u32x4{w[0], w[1], w[2], w[3]};
                }
                *reinterpret_cast<u32x4 *>(d + o) = v;
            }
        } else if (esz == 4) {                                     // a source that starts at an odd address: element-wise
            for (long o = lo + lane * 4L; o < hi; o += 64 * 4L)
                *reinterpret_cast<unsigned *>(d + o) = o < live ? *reinterpret_cast<const unsigned *>(src + o) : 0u;
        } else {
            for (long o = lo + lane * 2L; o < hi; o += 64 * 2L)
                *reinterpret_cast<unsigned short *>(d + o) = o < live ? *reinterpret_cast<const unsigned short *>(src + o) : (unsigned short)0;
        }
    }
}

// ---- G.711 recordings: gather AND expand ------------------------------------------------------------------------------
// The same gather for recordings that are still G.711 (vad_upload_rows_coded): a row is 1 byte a sample at ANY byte address --
// recordings packed back to back in an arena, 15 of 16 of them misaligned -- and leaves as int16 (g711_to_s16, device_api.hpp),
// so the link carries half the bytes of an int16 corpus.  rows[i].len = samples | codec << kRowCodecShift, codec wave-uniform per row;
// an S16 row is copied (2 bytes a sample, any EVEN address) and gives what gather_rows_kernel gives.
//
//   * the unit is the aligned 16-byte granule of the SOURCE.  With s = the row's first byte, m = s & 15 and A = s - m, lane l of
//     wave-load k reads granule A + lo + (64 k + l) 16: always an aligned vector, and only granules that hold a byte of the row
//     (such a granule cannot leave the row's page).  The 16 bytes a lane needs, [s + p, s + p + 16), are the upper 16 - m bytes of
//     its granule and the lower m of the NEXT one -- which the next lane holds: one ds_bpermute per dword (no LDS is allocated), a
//     v_alignbyte funnel per output dword.  Lane 63 takes lane 0 of the next wave-load, and the segment's last wave-load one extra
//     granule that lane 0 alone reads: 1 / 512 more bytes than an aligned row, no byte-wise loads anywhere.
//   * a segment is 8 KiB of source as above (8 x 16 B per lane in flight, non-temporal): 8 192 samples = 16 KiB of batch for a G.711
//     row, 4 096 samples for an S16 row; a vector of 16 codes leaves as two 16-byte stores;
//   * the segment that holds the row's end (and the padding behind it) takes the same loads one wave-load at a time; samples past the
//     row's length are zeroed AFTER the expansion -- padding is int16 zero, never an expanded pad byte (A-law has no code for 0).
//   * footprint as above: kGatherWaves one-wave workgroups for host sources, the wide grid for device sources.
constexpr long kRowLenMask = (1L << kRowCodecShift) - 1;
using u32x4 = unsigned __attribute__((ext_vector_type(4)));

// bytes [m, m + 16) of the 32 bytes c ++ n; m is wave-uniform
__device__ __forceinline__ u32x4 shift_bytes(u32x4 c, u32x4 n, int m) {
    const int dq = m >> 2;
    unsigned w0, w1, w2, w3, w4;
    if (dq == 0) {
        w0 = c.x, w1 = c.y, w2 = c.z, w3 = c.w, w4 = n.x;
    } else if (dq == 1) {
        w0 = c.y, w1 = c.z, w2 = c.w, w3 = n.x, w4 = n.y;
    } else if (dq == 2) {
        w0 = c.z, w1 = c.w, w2 = n.x, w3 = n.y, w4 = n.z;
    } else {
        w0 = c.w, w1 = n.x, w2 = n.y, w3 = n.z, w4 = n.w;
    }
    const unsigned r = (unsigned)m & 3u;                       // v_alignbyte_b32: ({hi, lo} >> 8 r) & 0xffffffff
    return u32x4{__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r), __builtin_amdgcn_alignbyte(w3, w2, r),
                 __builtin_amdgcn_alignbyte(w4, w3, r)};
}

// lane l <- lane l + 1's v; lane 63 <- `wrap`.  Every lane of the wave executes this.
__device__ __forceinline__ u32x4 next_lane(u32x4 v, u32x4 wrap, int lane) {
    u32x4 r{__shfl_down(v.x, 1u), __shfl_down(v.y, 1u), __shfl_down(v.z, 1u), __shfl_down(v.w, 1u)};
    return lane == 63 ? wrap : r;
}

__device__ __forceinline__ u32x4 lane0_of(u32x4 v) {
    return u32x4{(unsigned)__builtin_amdgcn_readfirstlane((int)v.x), (unsigned)__builtin_amdgcn_readfirstlane((int)v.y),
                 (unsigned)__builtin_amdgcn_readfirstlane((int)v.z), (unsigned)__builtin_amdgcn_readfirstlane((int)v.w)};
}

// four codes (one dword) -> four int16 in two dwords
template <int CODEC>
__device__ __forceinline__ void expand4(unsigned w, unsigned &lo, unsigned &hi) {
    auto one = [](unsigned code) -> unsigned {
        return (unsigned)(unsigned short)(CODEC == VAD_PCM_ULAW ? ulaw_to_s16((uint8_t)code) : alaw_to_s16((uint8_t)code));
    };
    lo = one(w & 0xffu) | one((w >> 8) & 0xffu) << 16;
    hi = one((w >> 16) & 0xffu) | one(w >> 24) << 16;
}

// The 16 source bytes x of one lane -> the batch row at source position p.  CODEC 0: a copy (16 bytes at d + p); else 16 codes -> 16
// int16 (32 bytes at d + 2 p).  keep: source bytes of x that belong to the row (>= 16: all), the rest leave as zeros; room: source
// bytes the row has left at p (16, or 8 at the end of a G.711 row whose width is 8 mod 16).  NT: non-temporal stores.
template <int CODEC, bool NT>
__device__ __forceinline__ void put_vector(u32x4 x, uint8_t *d, long p, long keep, long room) {
    auto store = [](u32x4 v, uint8_t *at) {
        if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(at));
        else *reinterpret_cast<u32x4 *>(at) = v;
    };
    if (CODEC == 0) {
        if (keep < 16) {
            unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long k = keep - 4 * i;
                w[i] = k >= 4 ? w[i] : k <= 0 ? 0u : w[i] & ((1u << (8 * (int)k)) - 1u);
            }
            x = u32x4{w[0], w[1], w[2], w[3]};
        }
        store(x, d + p);
    } else {
        unsigned o[8];
        expand4<CODEC>(x.x, o[0], o[1]);
        expand4<CODEC>(x.y, o[2], o[3]);
        expand4<CODEC>(x.z, o[4], o[5]);
        expand4<CODEC>(x.w, o[6], o[7]);
        if (keep < 16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long k = keep - 2 * j;
                o[j] = k >= 2 ? o[j] : k == 1 ? o[j] & 0xffffu : 0u;
            }
        }
        store(u32x4{o[0], o[1], o[2], o[3]}, d + 2 * p);
        if (room >= 16) store(u32x4{o[4], o[5], o[6], o[7]}, d + 2 * p + 16);
    }
}

// The 16 source bytes x of one lane, whole interleaved STEREO frames (source position p is a multiple of 16, a frame is 4 or 2 bytes)
// -> the two batch rows d0 (channel 0) and d1 (channel 1); a null row is a channel nobody wants.  keep as in put_vector: source bytes
// of x that belong to the recording, a whole number of frames; the samples behind them leave as int16 zeros (zeroed after the expansion).
// Every lane of the wave executes this (the S16 form trades halves with the neighbour lane); `on`: this lane's vector lies inside the
// row and is stored.
//   * G.711: 8 frames.  v_perm_b32 picks the even bytes (channel 0) and the odd ones (channel 1) of two dwords at a time; 8 codes of a
//     channel expand to 16 bytes: ONE 16-byte store per channel and lane, at byte p of the channel's row.
//   * S16: 4 frames = 8 bytes a channel.  v_perm_b32 picks the low halfwords (channel 0) and the high ones (channel 1); lanes 2 i and
//     2 i + 1 hold the 8 consecutive frames at p, so the even lane hands its channel-1 half to the odd one and takes the odd one's
//     channel-0 half (two DPP / bpermute moves): the even lane stores 16 bytes of channel 0, the odd lane 16 bytes of channel 1.
template <int CODEC, bool NT>
__device__ __forceinline__ void put_stereo(u32x4 x, uint8_t *d0, uint8_t *d1, long p, long keep, bool on, int lane) {
    auto store = [](u32x4 v, uint8_t *at) {
        if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(at));
        else *reinterpret_cast<u32x4 *>(at) = v;
    };
    if (CODEC == 0) {
        constexpr unsigned kLo = 0x05040100u, kHi = 0x07060302u;          // halfwords 0, 2 / 1, 3 of the 8 bytes {S0 : S1}
        unsigned l0 = __builtin_amdgcn_perm(x.y, x.x, kLo), l1 = __builtin_amdgcn_perm(x.w, x.z, kLo);
        unsigned r0 = __builtin_amdgcn_perm(x.y, x.x, kHi), r1 = __builtin_amdgcn_perm(x.w, x.z, kHi);
        if (keep < 16) {
            const long f = keep >> 2;                                    // frames of x that exist
            const unsigned m0 = f >= 2 ? ~0u : f == 1 ? 0xffffu : 0u, m1 = f >= 4 ? ~0u : f == 3 ? 0xffffu : 0u;
            l0 &= m0, r0 &= m0, l1 &= m1, r1 &= m1;
        }
        const bool odd = lane & 1;
        const unsigned g0 = __shfl_xor(odd ? l0 : r0, 1), g1 = __shfl_xor(odd ? l1 : r1, 1);
        uint8_t *d = odd ? d1 : d0;
        if (on && d) store(odd ? u32x4{g0, g1, r0, r1} : u32x4{l0, l1, g0, g1}, d + ((odd ? p - 16 : p) >> 1));
    } else {
        constexpr unsigned kEven = 0x06040200u, kOdd = 0x07050301u;      // bytes 0, 2, 4, 6 / 1, 3, 5, 7 of the 8 bytes {S0 : S1}
        unsigned o[8];
        expand4<CODEC>(__builtin_amdgcn_perm(x.y, x.x, kEven), o[0], o[1]);
        expand4<CODEC>(__builtin_amdgcn_perm(x.w, x.z, kEven), o[2], o[3]);
        expand4<CODEC>(__builtin_amdgcn_perm(x.y, x.x, kOdd), o[4], o[5]);
        expand4<CODEC>(__builtin_amdgcn_perm(x.w, x.z, kOdd), o[6], o[7]);
        if (keep < 16) {
            const long f = keep >> 1;                                    // frames of x that exist
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long k = f - 2 * j;
                const unsigned mk = k >= 2 ? ~0u : k == 1 ? 0xffffu : 0u;
                o[j] &= mk, o[4 + j] &= mk;
            }
        }
        if (on && d0) store(u32x4{o[0], o[1], o[2], o[3]}, d0 + p);
        if (on && d1) store(u32x4{o[4], o[5], o[6], o[7]}, d1 + p);
    }
}

// One (row, segment) item.  A: the aligned granule that holds the row's first byte, m: the first byte's place in it, live: source bytes
// of the row, wsb: source bytes of a full batch row (a multiple of 16 for a copy, of 8 for G.711), d: the batch row.
// CH = 2 (gather_channels_kernel): the source is interleaved stereo -- live and wsb count its bytes, 2 x those of a channel, so wsb is a
// multiple of 16 whatever the codec; the loads and the shuffle are the same, every vector leaves through put_stereo into d (channel 0)
// and d1 (channel 1).
template <int CODEC, int CH = 1>
__device__ __forceinline__ void move_segment(const uint8_t *A, int m, long live, long wsb, uint8_t *d, long lo, int lane,
                                             uint8_t *d1 = nullptr) {
    if (lo >= wsb) return;                                     // (a G.711 row has half the segments of an S16 row of its width)
    const u32x4 zero{0u, 0u, 0u, 0u};
    if (lo + kSegBytes <= live) {
        // a whole segment inside the recording: 8 wave-loads in flight (+ the one granule behind them when the row is misaligned:
        // m > 0 and lo + 8192 <= live, so it holds row bytes), then the stores
        u32x4 v[8], extra = zero;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(A + lo + (k * 64 + lane) * 16L));
        if (m) {
            if (lane == 0) extra = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(A + lo + kSegBytes));
            extra = lane0_of(extra);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = shift_bytes(v[k], next_lane(v[k], lane0_of(k < 7 ? v[k + 1] : extra), lane), m);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (CH == 1) put_vector<CODEC, true>(v[k], d, lo + (k * 64 + lane) * 16L, 16, 16);
            else put_stereo<CODEC, true>(v[k], d, d1, lo + (k * 64 + lane) * 16L, 16, true, lane);
        }
        return;
    }
    // the segment with the recording's end and / or the padding: one wave-load at a time.  Granule p is read iff it holds a byte of the
    // row: p < m + live.  A lane may read the granule BEHIND the segment's last vector (p < hi + 16) for its neighbour and stores
    // nothing there: a misaligned row's last vector ends in it.  That also holds where hi is 8 mod 16 (the end of a G.711 row whose width
    // is): the last vector starts at hi - 8, its 8 bytes end m + 8 bytes into its granule, past it when m > 8 -- and `p < end` still
    // admits the read only if that granule holds a byte of the row, which is the page guarantee.
    const long hi = lo + kSegBytes < wsb ? lo + kSegBytes : wsb;
    const long end = live > 0 ? m + live : 0;                  // granules at p >= end hold nothing of the row
    for (long base = lo; base < hi; base += 64 * 16L) {        // (wave-uniform trip count: next_lane needs every lane)
        const long p = base + lane * 16L;
        u32x4 c = zero, n = zero;
        if (p < end && p < hi + 16) c = *reinterpret_cast<const u32x4 *>(A + p);
        if (m) {
            if (lane == 63 && p < hi && p + 16 < end) n = *reinterpret_cast<const u32x4 *>(A + p + 16);
            c = shift_bytes(c, next_lane(c, n, lane), m);
        }
        if (CH == 1) {
            if (p < hi) put_vector<CODEC, false>(c, d, p, live - p, hi - p);
        } else {
            put_stereo<CODEC, false>(c, d, d1, p, live - p, p < hi, lane);     // (hi is a multiple of 32: a lane pair is inside or outside)
        }
    }
}

__global__ void __launch_bounds__(64) gather_expand_rows_kernel(const RowDesc *rows, long n, long width, uint8_t *dst, long segs_per_row) {
    const long items = n * segs_per_row;
    const int lane = threadIdx.x;
    __builtin_amdgcn_s_setprio(3);          // as in gather_rows_kernel
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long row = item / segs_per_row, lo = (item % segs_per_row) * kSegBytes;
        const size_t s = (size_t)rows[row].ptr;
        const long tag = rows[row].len, len = tag & kRowLenMask;
        const int codec = (int)(tag >> kRowCodecShift), m = (int)(s & 15);
        const uint8_t *A = reinterpret_cast<const uint8_t *>(s - m);
        uint8_t *d = dst + row * width * 2;
        if (codec == VAD_PCM_S16) move_segment<0>(A, m, len * 2, width * 2, d, lo, lane);
        else if (codec == VAD_PCM_ULAW) move_segment<VAD_PCM_ULAW>(A, m, len, width, d, lo, lane);
        else move_segment<VAD_PCM_ALAW>(A, m, len, width, d, lo, lane);
    }
}

// ---- interleaved stereo recordings: gather, expand AND split -------------------------------------------------------------
// The same gather over a table of SOURCES (vad_upload_rows_channels): a source is a recorded call as its WAV data chunk holds it, one
// or two channels interleaved frame by frame, S16 at any even address (a stereo frame may sit at 2 mod 4) or G.711 at any byte address,
// and every wanted channel leaves as one row of the int16 batch: src[i].dst[c] is the batch row of channel c, -1 a channel nobody
// wants.  The source crosses the link once, as it lies on disk; the de-interleaving that the host would otherwise do -- a strided byte
// pass over the whole corpus -- happens in the lanes' registers between the shuffle and the stores (put_stereo).  src[i].tag = frames |
// channels << kRowChanShift | codec << kRowCodecShift, all wave-uniform per source.
//   * a one-channel source is move_segment as gather_expand_rows_kernel calls it: the same loads, the same stores, the same bits;
//   * a two-channel source takes the same aligned granule loads and the same neighbour-lane shuffle on its interleaved bytes -- 16
//     source bytes at a multiple of 16 behind the first frame are whole frames -- and a segment is 8 KiB of SOURCE: 2 048 frames of
//     stereo S16, 4 096 of stereo G.711;
//   * the items are sized for the widest source of the table (frame_bytes: 4 for stereo S16); narrower ones leave their spare items
//     at once, as a G.711 row does in gather_expand_rows_kernel;
//   * footprint as above.  No LDS; 95 VGPRs, one more than gather_expand_rows_kernel (the whole-segment path holds its 8 vectors and the
//     granule behind them; a lane splits one vector at a time).
constexpr long kChanLenMask = (1L << kRowChanShift) - 1;

__global__ void __launch_bounds__(64) gather_channels_kernel(const ChanRowDesc *src, long n, long width, uint8_t *dst, long segs_per_row) {
    const long items = n * segs_per_row;
    const int lane = threadIdx.x;
    __builtin_amdgcn_s_setprio(3);          // as in gather_rows_kernel
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long row = item / segs_per_row, lo = (item % segs_per_row) * kSegBytes;
        const size_t s = (size_t)src[row].ptr;
        const long tag = src[row].tag, frames = tag & kChanLenMask;
        const int codec = (int)(tag >> kRowCodecShift), ch = (int)(tag >> kRowChanShift) & 0xff, m = (int)(s & 15);
        const int r0 = src[row].dst[0], r1 = src[row].dst[1];
        const uint8_t *A = reinterpret_cast<const uint8_t *>(s - m);
        uint8_t *d0 = r0 >= 0 ? dst + r0 * width * 2 : nullptr, *d1 = r1 >= 0 ? dst + r1 * width * 2 : nullptr;
        if (ch == 1) {
            if (!d0) continue;
            if (codec == VAD_PCM_S16) move_segment<0>(A, m, frames * 2, width * 2, d0, lo, lane);
            else if (codec == VAD_PCM_ULAW) move_segment<VAD_PCM_ULAW>(A, m, frames, width, d0, lo, lane);
            else move_segment<VAD_PCM_ALAW>(A, m, frames, width, d0, lo, lane);
        } else {
            if (!d0 && !d1) continue;
            if (codec == VAD_PCM_S16) move_segment<0, 2>(A, m, frames * 4, width * 4, d0, lo, lane, d1);
            else if (codec == VAD_PCM_ULAW) move_segment<VAD_PCM_ULAW, 2>(A, m, frames * 2, width * 2, d0, lo, lane, d1);
            else move_segment<VAD_PCM_ALAW, 2>(A, m, frames * 2, width * 2, d0, lo, lane, d1);
        }
    }
}

}  // namespace

hipError_t launch_gather_rows(const RowDesc *rows, long n, long width, int esz, void *dst, bool rows_on_device, hipStream_t s) {
    if (n <= 0 || width <= 0) return hipSuccess;
    const long wb = width * esz, segs = (wb + kSegBytes - 1) / kSegBytes;
    const long items = n * segs;
    if (items > 0x7fffffffL) return hipErrorInvalidValue;
    // sources in HBM (a packed window that one big DMA brought over): an HBM-to-HBM scatter, as wide as the chip -- it runs
    // for a fraction of a millisecond; sources in host memory: the narrow persistent grid described above
    const long waves = rows_on_device ? 4096 : kGatherWaves;
    const unsigned grid = (unsigned)(items < waves ? items : waves);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(64), 0, s, rows, n, wb, esz, static_cast<uint8_t *>(dst), segs);
    return hipGetLastError();
}

hipError_t launch_gather_expand_rows(const RowDesc *rows, long n, long width, void *dst_i16, bool rows_on_device, hipStream_t s) {
    if (n <= 0 || width <= 0) return hipSuccess;
    // The items are sized for an S16 row (2 source bytes a sample), whatever the table holds: a G.711 row uses the first half of its
    // items and leaves the others at once (move_segment: lo >= wsb), at the price of reading its table entry once more -- 16 bytes
    // over PCIe per 8 KiB segment for host sources, nothing that shows for device sources.
    const long segs = (width * 2 + kSegBytes - 1) / kSegBytes;
    const long items = n * segs;
    if (items > 0x7fffffffL) return hipErrorInvalidValue;
    const long waves = rows_on_device ? 4096 : kGatherWaves;      // (as launch_gather_rows)
    const unsigned grid = (unsigned)(items < waves ? items : waves);
    hipLaunchKernelGGL(gather_expand_rows_kernel, dim3(grid), dim3(64), 0, s, rows, n, width, static_cast<uint8_t *>(dst_i16), segs);
    return hipGetLastError();
}

hipError_t launch_gather_channels(const ChanRowDesc *src, long n, long width, int frame_bytes, void *dst_i16, bool rows_on_device,
                                  hipStream_t s) {
    if (n <= 0 || width <= 0) return hipSuccess;
    const long segs = (width * frame_bytes + kSegBytes - 1) / kSegBytes;      // (of the table's widest kind of source)
    const long items = n * segs;
    if (items > 0x7fffffffL) return hipErrorInvalidValue;
    const long waves = rows_on_device ? 4096 : kGatherWaves;      // (as launch_gather_rows)
    const unsigned grid = (unsigned)(items < waves ? items : waves);
    hipLaunchKernelGGL(gather_channels_kernel, dim3(grid), dim3(64), 0, s, src, n, width, static_cast<uint8_t *>(dst_i16), segs);
    return hipGetLastError();
}

}  // namespace vad
