// collector.hpp -- which samples of a recording a segment list keeps, written once for the host twin (segmenter.cpp,
// vad_collect_segments) and for the device gather (kernel_collect.hip).
//
// Semantics are those of collect_chunks / drop_chunks (reference src/silero_vad/utils_vad.py:552-655) on the 16 kHz signal of
// `len` samples: the output is the concatenation of PARTS, each a run [a, b) of the signal's samples.
//   invert 0 (collect_chunks): part k = segment k, for k < n.
//   invert 1 (drop_chunks):    part k = what lies between the end of segment k - 1 (0 for k = 0) and the start of segment k (len for
//                              k = n), for k <= n.
// A segment is clamped to [0, len] first and one whose end lies in front of its start is empty (it ends where it starts); a part
// with b <= a is empty.  For the segment lists the scan produces -- ordered, disjoint, inside the signal -- that is the reference
// bit for bit; for anything else it is the reference's slicing with indices confined to the signal.
#pragma once
#include <cstdint>

#include "../../include/silero_vad_hip.h"

#if defined(__HIPCC__)
#define VAD_COLLECT_HD __host__ __device__
#else
#define VAD_COLLECT_HD
#endif

namespace vad {

struct Part {
    int64_t a, b;
};

VAD_COLLECT_HD inline int64_t clamp_sample(int64_t v, int64_t len) { return v < 0 ? 0 : v > len ? len : v; }

VAD_COLLECT_HD inline long collect_parts(long n, int invert) { return invert ? n + 1 : n; }

VAD_COLLECT_HD inline Part collect_part(const vad_segment *segs, long n, long k, int64_t len, int invert) {
    if (!invert) return Part{clamp_sample(segs[k].start, len), clamp_sample(segs[k].end, len)};
    int64_t a = 0;
    if (k > 0) {
        const int64_t s = clamp_sample(segs[k - 1].start, len), e = clamp_sample(segs[k - 1].end, len);
        a = e > s ? e : s;
    }
    return Part{a, k < n ? clamp_sample(segs[k].start, len) : len};
}

// samples of a row that the batch can hold: sample s of the 16 kHz signal is element s * step of a row of ld elements
VAD_COLLECT_HD inline int64_t row_samples(int64_t audio_len, long ld, int step) {
    return clamp_sample(audio_len, (ld + step - 1) / step);
}

}  // namespace vad
