// tape.hpp -- which samples of a live stream the pump's tape still holds, written once for the host (pump.hip: vad_tape_window,
// vad_pump_tape_window, vad_pump_fetch_audio; vad_tape_run and the version 3 snapshots) and for the device (kernel_tape.hip).
//
// The tape of a stream is a ring of `chunks` chunks of N samples (int16, or float32: nothing here depends on the element).  Two counters describe it: `count`, the chunks stepped since the
// stream's clock started (vad_pump_open, or the chunk an import continued at), and `floor`, the first chunk the tape can hold (0 after
// an open; the chunk an import continued at).  Chunk k lies in ring slot k % chunks, so sample s of the stream's clock lies at element
// s % (chunks * N) of its ring, and the tape holds the samples
//     [held_lo, held_hi),  held_lo = max(floor, count - chunks) * N,  held_hi = count * N.
// A request [start, end), start <= end, of any int64 values is confined to that window -- every clamp comes before a subtraction:
//     first = min(max(start, held_lo), held_hi),  last = min(max(end, first), held_hi),  n = last - first.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VAD_TAPE_HD __host__ __device__
#else
#define VAD_TAPE_HD
#endif

namespace vad {

VAD_TAPE_HD inline int64_t tape_held_lo(int64_t count, int64_t floor, int64_t chunks, int64_t N) {
    const int64_t oldest = count - chunks;
    return (floor > oldest ? floor : oldest) * N;
}

VAD_TAPE_HD inline int64_t tape_held_hi(int64_t count, int64_t N) { return count * N; }

VAD_TAPE_HD inline int64_t tape_first(int64_t start, int64_t held_lo, int64_t held_hi) {
    const int64_t a = start > held_lo ? start : held_lo;
    return a < held_hi ? a : held_hi;
}

VAD_TAPE_HD inline int64_t tape_last(int64_t end, int64_t first, int64_t held_hi) {
    const int64_t b = end > first ? end : first;
    return b < held_hi ? b : held_hi;
}

// [start, end) confined to the window of (count, floor): its first held sample and the number of held samples
VAD_TAPE_HD inline void tape_window(int64_t count, int64_t floor, int64_t chunks, int64_t N, int64_t start, int64_t end, int64_t *first,
                                    int64_t *n) {
    const int64_t lo = tape_held_lo(count, floor, chunks, N), hi = tape_held_hi(count, N);
    const int64_t a = tape_first(start, lo, hi);
    *first = a;
    *n = tape_last(end, a, hi) - a;
}

// The RUN a snapshot carries (blob version 3): the whole chunks from the one that holds sample `from` to the newest one, as far as the
// tape holds them (floor >= 0, so held_lo >= 0).  `from` is clamped into [held_lo, held_hi] BEFORE it is divided, so any int64 is safe;
// a position in the middle of a chunk rounds down to its chunk.
//     first_chunk = min(max(from / N, held_lo / N), count),  n_chunks = count - first_chunk
VAD_TAPE_HD inline void tape_run(int64_t count, int64_t floor, int64_t chunks, int64_t N, int64_t from, int64_t *first_chunk, int64_t *n_chunks) {
    const int64_t a = tape_first(from, tape_held_lo(count, floor, chunks, N), tape_held_hi(count, N));
    *first_chunk = a / N;
    *n_chunks = count - a / N;
}

// the ring slot chunk k of a stream is taped into (k >= 0)
VAD_TAPE_HD inline int64_t tape_slot(int64_t k, int64_t chunks) { return (int64_t)((uint64_t)k % (uint64_t)chunks); }

// the element of a stream's ring that holds sample s of its clock (s >= 0)
VAD_TAPE_HD inline int64_t tape_element(int64_t s, int64_t chunks, int64_t N) { return (int64_t)((uint64_t)s % (uint64_t)(chunks * N)); }

}  // namespace vad
