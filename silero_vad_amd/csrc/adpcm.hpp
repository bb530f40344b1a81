// adpcm.hpp -- DVI4 (RFC 3551 section 4.5.1: 4-bit IMA ADPCM with the decoder's state in a 4-byte header), the one definition the pump's
// assembly kernels (kernel_present.hip) and the host export vad_adpcm_expand (pump.hip) share.  Plain C++ on the host, __host__
// __device__ under hipcc; integer arithmetic only.
//
// A payload is {predict: int16 big-endian, index: uint8 (above 88: used as 88), reserved: ignored, then 4-bit codes, two a byte, the
// first sample in the HIGH nibble}; nbytes bytes hold 2 * (nbytes - 4) samples.  One code d with the state (pred, idx):
//   step = STEP[idx];  v = (step >> 3) + (d & 4 ? step : 0) + (d & 2 ? step >> 1 : 0) + (d & 1 ? step >> 2 : 0)
//   pred = clamp(d & 8 ? pred - v : pred + v, -32768, 32767);  idx = clamp(idx + IDX[d & 7], 0, 88);  the sample is pred
// -- the values of Python's audioop.adpcm2lin(payload[4:], 2, (predict, min(index, 88))).
//
// The recurrence as two scans (the device form).  Both updates are saturating adds, x -> min(hi, max(lo, x + a)), and those are closed
// under composition: adpcm_then below.  The step index does not depend on the predictor, so a scan over (IDX[d & 7], 0, 88) gives every
// sample's index, the steps give every sample's +-v, and a scan over (+-v, -32768, 32767) gives the samples.  Over 512 samples |a| stays
// below 512 * 61 438 < 2^25 and lo / hi are sums of two such values: 32 bits hold them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VAD_ADPCM_HD __host__ __device__
#else
#define VAD_ADPCM_HD
#endif

namespace vad {

constexpr int kAdpcmHeader = 4;                  // bytes in front of a payload's codes
constexpr int kAdpcmSteps = 89;
constexpr int kAdpcmMaxIndex = kAdpcmSteps - 1;

VAD_ADPCM_HD inline int adpcm_step_of(int idx) {
    constexpr int16_t kStep[kAdpcmSteps] = {
        7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,    31,    34,    37,
        41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,   130,   143,   157,   173,   190,   209,
        230,   253,   279,   307,   337,   371,   408,   449,   494,   544,   598,   658,   724,   796,   876,   963,   1060,  1166,
        1282,  1411,  1552,  1707,  1878,  2066,  2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,
        7132,  7845,  8630,  9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
    return kStep[idx];
}
// IDX[d & 7] = {-1, -1, -1, -1, 2, 4, 6, 8}
VAD_ADPCM_HD inline int adpcm_index_add(unsigned d) { return d & 4u ? 2 * (int)(d & 3u) + 2 : -1; }
// the signed change of the predictor that code d asks for at step size `step`
VAD_ADPCM_HD inline int adpcm_delta(int step, unsigned d) {
    const int v = (step >> 3) + (d & 4u ? step : 0) + (d & 2u ? step >> 1 : 0) + (d & 1u ? step >> 2 : 0);
    return d & 8u ? -v : v;
}
VAD_ADPCM_HD inline int adpcm_clamp(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }
// the header's two fields, from its bytes in wire order
VAD_ADPCM_HD inline int adpcm_header_predict(unsigned b0, unsigned b1) { return (int)(int16_t)(uint16_t)((b0 & 0xffu) << 8 | (b1 & 0xffu)); }
VAD_ADPCM_HD inline int adpcm_header_index(unsigned b2) { return (int)(b2 & 0xffu) > kAdpcmMaxIndex ? kAdpcmMaxIndex : (int)(b2 & 0xffu); }
// code j of a payload's code bytes: two a byte, the first in the high nibble
VAD_ADPCM_HD inline unsigned adpcm_code(const uint8_t *codes, long j) { return (codes[j >> 1] >> (j & 1 ? 0 : 4)) & 15u; }

// x -> min(hi, max(lo, x + a))
struct AdpcmSat {
    int a, lo, hi;
};
constexpr int kAdpcmWide = 1 << 20;              // the identity's bounds: no predictor, index or partial sum of one row's piece reaches them
VAD_ADPCM_HD inline AdpcmSat adpcm_identity() { return AdpcmSat{0, -kAdpcmWide, kAdpcmWide}; }
VAD_ADPCM_HD inline int adpcm_apply(const AdpcmSat &f, int x) { return adpcm_clamp(x + f.a, f.lo, f.hi); }
// g after f
VAD_ADPCM_HD inline AdpcmSat adpcm_then(const AdpcmSat &f, const AdpcmSat &g) {
    return AdpcmSat{f.a + g.a, adpcm_clamp(f.lo + g.a, g.lo, g.hi), adpcm_clamp(f.hi + g.a, g.lo, g.hi)};
}

// The serial decode (the host twin; the kernels scan): out[0 .. 2 * (nbytes - 4)) <- the payload's samples; -> their number.
// nbytes == 4: a header alone, 0 samples, neither pointer is looked at.  nbytes < 4, or a null pointer with nbytes > 4: -1, nothing
// touched.
inline long adpcm_expand_serial(const uint8_t *payload, long nbytes, int16_t *out) {
    if (nbytes < kAdpcmHeader) return -1;
    if (nbytes == kAdpcmHeader) return 0;
    if (!payload || !out) return -1;
    int pred = adpcm_header_predict(payload[0], payload[1]), idx = adpcm_header_index(payload[2]);
    const long n = 2 * (nbytes - kAdpcmHeader);
    for (long j = 0; j < n; ++j) {
        const unsigned d = adpcm_code(payload + kAdpcmHeader, j);
        pred = adpcm_clamp(pred + adpcm_delta(adpcm_step_of(idx), d), -32768, 32767);
        idx = adpcm_clamp(idx + adpcm_index_add(d), 0, kAdpcmMaxIndex);
        out[j] = (int16_t)pred;
    }
    return n;
}

}  // namespace vad
