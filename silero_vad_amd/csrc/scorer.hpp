// scorer.hpp -- the validation scores: what one chunk (a float32 probability and a uint8 label) contributes to the masked BCE loss and
// to the pooled ROC-AUC of a labelled validation set (reference validate(), tuning/utils.py:252-298).  Written once for the host
// (segmenter.cpp, vad_chunk_scores_host / vad_auc_counts_host) and for the device (kernel_score.hip).
//
// Validity: a chunk is VALID when its label is 0 or 1 and 0 <= p <= 1.  A NaN fails both comparisons; -0.0f passes and is taken as
// +0.0f.  A label above 1 (VAD_LABEL_IGNORE) is a chunk that is not there (the reference's mask 0).  A label of 0 / 1 with any other
// probability is BAD: it is counted, it enters no sum and it gets no key -- nn.BCELoss rejects such an input outright.
//
// The BCE term is nn.BCELoss's arithmetic with the log in double: the reference computes 1 - p in fp32 and clamps the log at -100.
//   label 1: -max(log((double)p), -100)        label 0: -max(log((double)(1.0f - p)), -100)
//
// The key orders the valid chunks of a whole corpus by probability without a payload: with v the bit pattern of p (non-negative
// floats order like their bits; v <= 0x3F800000 < 2^30), key = (v << 1) | label.  Everything else is VAD_SCORE_KEY_NONE.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/silero_vad_hip.h"

#if defined(__HIPCC__)
#define VAD_SCORE_HD __host__ __device__
#else
#define VAD_SCORE_HD
#endif

namespace vad {

enum ScoreKind : int { kScoreAbsent = 0, kScoreNeg = 1, kScorePos = 2, kScoreBad = 3 };

struct ScoreChunk {
    uint32_t key;      // (v << 1) | label, or VAD_SCORE_KEY_NONE
    int kind;          // ScoreKind
    double term;       // the BCE term of a valid chunk, else 0
};

VAD_SCORE_HD inline uint32_t score_bits(float p) {
    uint32_t v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __float_as_uint(p);
#else
    std::memcpy(&v, &p, sizeof v);
#endif
    return v & 0x7FFFFFFFu;                                   // -0.0f is +0.0f; nothing else that is valid has the sign bit
}

VAD_SCORE_HD inline ScoreChunk score_chunk(float p, unsigned label) {
    ScoreChunk c{VAD_SCORE_KEY_NONE, kScoreAbsent, 0.0};
    if (label > 1u) return c;
    if (!(p >= 0.0f && p <= 1.0f)) {
        c.kind = kScoreBad;
        return c;
    }
    const float q = label ? p : 1.0f - p;
    const double l = log((double)q);                          // -inf at q = 0: clamped
    c.term = 0.0 - (l > -100.0 ? l : -100.0);                 // (0.0 - x: a plain zero at q = 1, not -0.0)
    c.kind = label ? kScorePos : kScoreNeg;
    c.key = (score_bits(p) << 1) | label;
    return c;
}

// The pooled rank statistic, fed with the non-NONE keys in ascending order: for equal v the negatives (low bit 0) come first.
struct AucWalk {
    uint64_t u2 = 0, n_pos = 0, n_neg = 0;
    uint64_t neg_below = 0, neg_eq = 0;
    uint32_t v = 0xFFFFFFFFu;                                 // no key has this v (31 bits)

    void feed(uint32_t key) {
        const uint32_t kv = key >> 1;
        if (kv != v) {
            neg_below += neg_eq;
            neg_eq = 0;
            v = kv;
        }
        if (key & 1u) {
            u2 += 2 * neg_below + neg_eq;
            ++n_pos;
        } else {
            ++neg_eq;
            ++n_neg;
        }
    }
};

}  // namespace vad
