// sweeper.hpp -- the threshold sweep: per-chunk speech probabilities and 0 / 1 labels -> the confusion counts of the hysteresis
// decision, for one (enter, exit) threshold pair.  Written once for the host (segmenter.cpp, vad_threshold_counts_host) and for the
// device (kernel_sweep.hip, one lane per pair).
//
// Semantics are those of the inner loops of calculate_best_thresholds (reference tuning/utils.py:334-348): the decision starts at
// "not speech", a chunk with p >= enter switches it on, else one with p <= exit switches it off, anything between holds it -- and
// so does a NaN, for which both comparisons are false, as in Python.  The decision AFTER the chunk is scored against the chunk's
// label.  A label other than 0 / 1 (VAD_LABEL_IGNORE) is a chunk that is not there: it is skipped, the decision is untouched and
// nothing is counted (the reference's `predict` drops masked chunks before the loop, tuning/utils.py:317-319).
//
// The reference compares a float32 probability, widened to double, with a float64 grid value.  double(p) >= e holds exactly when
// p >= the smallest float32 that is >= e, and double(p) <= x exactly when p <= the largest float32 that is <= x: the caller rounds
// `enter` UP and `exit` DOWN to float32 (silero_vad_amd.threshold_pairs) and the comparisons here are fp32, with the same outcome.
// Any pair is accepted; exit >= enter is well defined by the order of the two tests.
#pragma once
#include <cstdint>

#include "../../include/silero_vad_hip.h"

#if defined(__HIPCC__)
#define VAD_SWEEP_HD __host__ __device__
#else
#define VAD_SWEEP_HD
#endif

namespace vad {

struct SweepCell {
    bool s = false;
    int tp = 0, tn = 0;

    // The only branches are on the label, which all pairs of a chunk share: the host's inner loop over the pairs is unswitched on
    // it, on the device (one pair per lane) they are scalar branches.  The decision itself is two compares and mask logic:
    // "on" wins over "off" as the reference's if / elif does, and a NaN, for which both are false, leaves s as it is.
    VAD_SWEEP_HD void feed(float p, unsigned label, float enter, float exit) {
        if (label > 1u) return;
        s = (p >= enter) | (s & !(p <= exit));
        if (label) tp += s;
        else tn += !s;
    }
};

// what a row's labels alone decide: n_pos (labels equal to 1) and n_valid (labels equal to 0 or 1)
struct SweepLabels {
    int n_pos = 0, n_valid = 0;

    VAD_SWEEP_HD void feed(unsigned label) {
        n_pos += label == 1u;
        n_valid += label <= 1u;
    }
};

}  // namespace vad
