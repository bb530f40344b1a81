// pump.hip -- vad_pump: BASELINE configs[4] as a native object.  `streams` live streams on one GPU, one tick = one 32 ms chunk of every
// stream: int16 audio lies in a page-locked ingest ring the audio sources write into, a tick is H2D -> the fused step kernel ->
// probabilities stored by the kernel straight into page-locked host memory -> VADIterator logic of every stream -> events.  No
// Python, no torch: what the reference's native streaming clients are around ONNX Runtime -- a tight loop of session.run per chunk
// with explicit state and the iterator logic inline (examples/cpp/silero-vad-onnx.cpp:335-390; Python twin
// src/silero_vad/utils_vad.py:507-549) -- for thousands of streams in lock step.
//
// Overlap is EXPLICIT, not left to which hardware queue the runtime hands a stream:
//   * three named HIP streams.  `copy[0]` / `copy[1]` carry nothing but the H2D copies of the even / odd ticks -- the link is the
//     scarce resource (8.4 MB per tick of 8 192 16 kHz streams, 146 us at 57 GB/s, against ~66 us of kernel).  `compute` carries
//     nothing but the step kernels, in tick order (the carried state demands that order anyway).  Two copy streams because a copy
//     engine leaves the link idle for ~17 us between two dependent copies of ONE stream (measured: profiles/r05_pump.md, 0.80 of the
//     link with two copies per tick on one stream); copies of consecutive ticks have no dependence on each other, and with two or more
//     ticks in flight the second engine's copy is already moving while the first one's successor is being set up;
//   * a tick may be cut into `parts` sub-batches of whole 16-stream tiles.  Part k's kernel waits for part k's copy BY EVENT
//     (h2d_done[buffer][k]); part k + 1's copy is already running beside it.  One part is the default: a second copy costs another
//     setup gap and buys ~15 us of latency;
//   * the device batch has THREE buffers ([3][streams][N] int16): tick t + 3's copies wait BY EVENT for tick t's kernels
//     (batch_free[buffer]) before they overwrite what those read.  Three, not two: the link idles with only two ticks in flight (copy ->
//     kernel -> host -> next copy: 70 us in every 370, rocprofv3 copy trace), and with two buffers the third tick's copy would wait on the
//     device for an event that is still open when it is issued.  With three buffers and three ticks in flight no copy has an open
//     dependency: same-lease A/B +13 % at 8 kHz, +0.5-1.3 % at 16 kHz, never slower (profiles/r06_pump_three_buffers.md);
//   * the context is ping-ponged between two device buffers (vad_step_split: the kernel writes the next context beside the one it
//     reads), so a tick is exactly `parts` copies and `parts` kernels -- no D2D blit of the context, no D2H operation;
//   * a ring slot may be rewritten by its sources as soon as the tick that read it has been retired (vad_pump_poll), and is refused
//     (VAD_ERR_ARG) while that tick is in flight.
//
// Streams that have no chunk this tick (vad_pump_submit_present): in the reference a stream is stepped when ITS caller has a chunk
// (utils_vad.py:507-549: one model call per arrived chunk; silero-vad-onnx.cpp:335-390), so a live stream whose packet is late must
// come out of the tick untouched.  Every ring slot starts with a header of `streams` flag bytes (page-locked, in front of the audio,
// so that flags + audio are ONE H2D copy); a masked tick copies the header along, the step kernels skip the absent rows' (h, c) and
// probability, kernel_present.hip carries their contexts over (vad_step_present), and vad_pump_poll leaves their iterator counters
// alone.  An unmasked tick copies no header and runs exactly the kernels it always ran.
//
// COMPACT ticks (vad_pump_submit_compact): the absent streams' rows need not cross the link at all.  The sources write the chunks of
// the streams that deliver back to back at the start of the slot (row i = the i-th delivering stream, ascending); the tick copies
// [position table | flags | those rows] in ONE copy into a second pair of device buffers, and a row-expansion pass on the compute
// stream (kernel_present.hip expand_rows: HBM to HBM, ~8 MB at most, a few us) puts every row where the step kernels read it.  The
// link cost of a tick then falls with the delivery rate; everything behind the expansion is the masked tick, bit for bit.
//
// PACKET ticks (vad_pump_submit_packets): receive paths deliver 10 / 20 / 30 ms frames of any length up to N, not chunks.  Row i of the
// slot's sample area is a packet of stream_of_row[i] at a 16-byte aligned offset; the host knows every length at submit time, so it
// keeps each stream's pending count, writes a row table {stream, offset, length, pending before} in front of the flags and sets the flag
// of every stream whose pending samples reach N.  ONE copy carries [row table | flags | packet samples] into the compact buffers, and
// kernel_present.hip assemble_packets splices each completing stream's batch row from its device carry and the packet head (and keeps
// the tail as the new carry) in place of expand_rows; everything behind it is the masked tick, bit for bit.  The chunk routes refuse a
// stream with pending samples; while no stream has any, they run exactly as before.  vad_pump_submit_coded_packets: the same tick with
// rows that may be G.711 mu-law / A-law (1 byte a sample, byte offsets); a tick with such a row takes assemble_coded_packets, which
// expands them to int16 on the device, and the carry holds int16 whatever the packets were.  A row may also be DVI4 (VAD_PCM_DVI4:
// a 4-byte header with the decoder's state, then 4-bit IMA ADPCM codes -- 4 + len / 2 bytes); a tick with such a row takes
// assemble_adpcm_packets, which decodes it by two wave scans (adpcm.hpp), and a burst tick with one the ADPCM form of assemble_burst.
// The pump takes such rows once vad_pump_set_adpcm has said so; until then codec 3 is the bad codec it always was.
// Every packet carries its own state: nothing is kept per stream, and the carry, the tape and a snapshot see int16 as before.
//
// BURST ticks (vad_pump_set_burst + vad_pump_submit_burst): a stream may have several rows in a tick and a row may be longer than N (a 60 ms
// Opus frame; what a jitter buffer releases after a stall), so a stream may complete k <= max_chunks chunks.  The host groups the rows by
// stream (a counting sort, arrival order kept) and writes k into the stream's flag byte -- every step kernel tests the flag as != 0, so
// the count IS sub-step 0's flag; kernel_present.hip assemble_burst (one wave per stream) cuts carry ++ rows into chunks: chunk 0 into the
// batch row, chunk j >= 1 into row b of d_more[j - 1], and burst_flags derives flags_j[b] = k[b] > j.  The tick then runs max(1, largest
// k) masked steps back to back on the compute stream, sub-step j over d_more[j - 1] with its probabilities in h_prob_more.  d_more and its
// flag rows are written and read on the compute stream only, in order: one buffer, not three.  Still ONE copy per tick.
//
// WIDE packet ticks (vad_pump_set_wideband + vad_pump_submit_wide_packets): WebRTC and Opus decoders deliver 32 / 48 kHz PCM.  A second
// page-locked ring of wide slots ([row table | flags | streams * N * max_step int16]) and its device landing buffers take rows sampled at
// step x 16 kHz; the host keeps each stream's comb phase beside its pending count and writes the row's first kept sample into the row
// table, and kernel_present.hip assemble_wide_packets keeps every step-th sample (the reference's x[::step]) on the way into the carry /
// the batch row.  The carry holds decimated int16: a stream may change route from tick to tick.  Still ONE copy per tick; everything
// behind the assembly is the masked tick, bit for bit.
//
// RESAMPLED packet ticks (vad_pump_set_resample + vad_pump_submit_resampled_packets): voice-agent and speech-synthesis APIs deliver 24 kHz
// PCM, desktop and browser capture 44.1 / 22.05 kHz.  A third page-locked ring of resample slots ([row table, 32 bytes a row | flags |
// streams * A int16], A = a chunk's input samples at the largest enabled rate) and its device landing buffers take int16 rows at up to
// four source rates; the host runs the streaming rule of the resampler per row (kernel_resample.hip resample_stream_ready: a stream that
// has received g inputs has emitted the outputs whose K inputs have all arrived), keeps each stream's bound rate, its input and output
// counters less whole periods and its fp32 pending count, and writes every index the kernel needs into the row table;
// kernel_present.hip assemble_resampled_packets runs the filter over history ++ row, splices the outputs behind the stream's fp32 carry
// and fills the ONE fp32 batch (compute stream only, like d_more), which the masked step then reads with elem_size 4.  A stream is
// BOUND to its rate from its first resampled row to vad_pump_open / vad_pump_close, and while it is, every other route refuses it: the
// int16 carry and the fp32 carry never hold samples of one stream at once.  Still ONE copy per tick.
//
// Waits block.  A source thread of a real server sleeps in its socket; the source threads of vad_pump_play, and its server loop, spin
// for at most 20 us on the counter they wait for and then sleep on it (futex), whatever the CPU budget: one of eight ranks under a
// 16-CPU quota has two CPUs for a server loop, a source thread and the HIP runtime's own threads, and a spinning (or yielding) thread
// there costs the tick it is waiting for (profiles/r06_pump_one_of_eight.md).
#include <hip/hip_runtime.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <thread>
#include <vector>

#include "../../include/silero_vad_hip.h"
#include "adpcm.hpp"
#include "device_api.hpp"
#include "host_threads.hpp"
#include "tape.hpp"

struct vad_pump {
    vad_engine *eng = nullptr;                   // a clone of the caller's engine: the pump's calls never touch the caller's scratch
    int device = 0, sr = 16000, N = 512, C = 64;
    int streams = 0, parts = 2, R = 4;
    std::vector<int> lo, hi;                     // part k = streams [lo[k], hi[k])
    double threshold = 0.5, min_silence = 1600, pad = 480;

    // a ring slot / a device batch buffer: [htab bytes][hpos bytes: int32 pos[streams], padded][hdr bytes: present[streams], padded]
    // [streams][N] int16 (the position table is written and copied by compact ticks only: it lies in FRONT of the flags so that a masked
    // tick's one copy starts at the flags and a compact tick's one copy at the table; a packet tick's row table, 16 bytes per row, ends
    // where the flags start and may reach back over the position table into htab)
    size_t htab = 0, hpos = 0, hdr = 0, slot_bytes = 0;
    uint8_t *h_ring = nullptr;                   // [R] slots, page-locked ingest ring
    float *h_prob = nullptr;                     // [R][streams]      page-locked, mapped: the kernels store here
    float *d_prob = nullptr;                     // device alias of h_prob
    static constexpr int NB = 3;                 // device batch buffers
    int nb = NB;                                 // ... in use (A/B knob SILERO_VAD_AMD_PUMP_BUFFERS=2: profiles/r06_pump_three_buffers.md)
    uint8_t *d_batch = nullptr;                  // [NB] device batch buffers (same layout as a ring slot)
    uint8_t *d_compact = nullptr;                // [NB] the same again: where a compact / packet tick's copy lands
    int16_t *d_carry = nullptr;                  // [streams][N] the pending samples of every stream (packet ticks; in place)
    float *d_ctx[2] = {nullptr, nullptr};        // [streams][C]      ping-pong
    std::vector<float *> d_state;                // per part: [2][hi - lo][128]
    hipStream_t copy[2] = {nullptr, nullptr}, compute = nullptr;    // copy[t & 1]: the copies of tick t
    std::vector<hipEvent_t> h2d_done[NB];        // [buffer][part]
    hipEvent_t batch_free[NB] = {nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> tick_done;           // [R]
    bool batch_used[NB] = {false, false, false};

    long ticks = 0;                              // ticks submitted so far (tick t: batch buffer t % NB, copy stream t & 1)
    long flips = 0;                              // steps submitted so far (step s: context s & 1 -> (s + 1) & 1); == ticks until a burst tick runs several
    long retired = 0;                            // ticks retired so far (vad_pump_poll)
    struct Flight { int r; bool masked; int steps = 1; };      // steps: the masked steps the tick ran (a burst tick: up to max_burst)
    std::deque<Flight> inflight;                 // the submitted, not yet retired ticks, oldest first
    std::vector<uint8_t> slot_busy;              // [R]
    // VADIterator state of every stream (utils_vad.py:500-503)
    std::vector<uint8_t> active, triggered, feed_mask;
    std::vector<int64_t> temp_end, current;
    // open / close take effect on the HOST side (iterator reset, active flag) at the tick they were issued before: ticks submitted
    // earlier are still in flight and belong to the slot's previous occupant
    struct Op { long at_tick; int stream; bool open; };
    std::deque<Op> pending;
    std::vector<long> src_pos;                   // vad_pump_play with a presence pattern: chunks stream b has delivered so far
    std::vector<int32_t> held;                   // [streams] samples submitted in packets and not yet stepped (host bookkeeping)
    long n_held = 0;                             // streams with held[b] > 0: the chunk routes check for them only while this is not 0
    std::vector<uint8_t> seen;                   // [streams] scratch of the packet-row validation (all zero between calls)
    // burst ticks (vad_pump_set_burst; max_burst == 0: not enabled, none of this is allocated)
    int max_burst = 0;                           // chunks a stream may complete in one tick
    bool adpcm = false;                          // vad_pump_set_adpcm: the coded packet and burst routes take VAD_PCM_DVI4 rows
    int16_t *d_more = nullptr;                   // [max_burst - 1][streams][N] the batch rows of sub-steps 1 ... (compute stream only)
    uint8_t *d_more_flags = nullptr;             // [max_burst - 1][hdr]        their flag rows
    float *h_prob_more = nullptr;                // [R][max_burst - 1][streams] page-locked, mapped: their probabilities
    float *d_prob_more = nullptr;                // device alias of h_prob_more
    std::vector<int> slot_steps;                 // [R] the steps the slot's last tick ran
    std::vector<int32_t> b_len, b_cnt, b_pos;    // [streams] scratch of build_burst: new samples, rows, next table row (b_len, b_cnt: zero between calls)
    std::vector<int32_t> b_touched;              // the streams a burst tick lists, by first appearance
    struct Held { int32_t stream, now; };
    std::vector<Held> b_new;                     // ... and what each has pending after the tick
    // wide packet ticks (vad_pump_set_wideband; max_step == 0: not enabled, none of this is allocated)
    int max_step = 0;                            // the largest decimation step a row may have (2: 32 kHz, 3: 48 kHz)
    // a wide slot / a wide landing buffer: [wtab bytes: the row table, ending where the flags start][hdr bytes: present[streams], padded]
    // [streams][N * max_step] int16
    size_t wtab = 0, wide_bytes = 0;
    uint8_t *h_wide = nullptr;                   // [R] wide slots, page-locked
    uint8_t *d_wide = nullptr;                   // [NB] where a wide tick's copy lands
    std::vector<uint8_t> w_step, w_phase;        // [streams] the step of the stream's last wide row (0: none yet) and its comb phase (host bookkeeping)
    struct Comb { int32_t stream, now; uint8_t step, phase; };
    std::vector<Comb> w_new;                     // what each listed stream has pending, and its step and phase, after the tick
    // resampled packet ticks (vad_pump_set_resample; n_rates == 0: not enabled, none of this is allocated)
    int n_rates = 0;
    int rates[vad::kMaxPumpRates] = {0, 0, 0, 0};                               // the enabled source rates, by rate index
    std::shared_ptr<const vad::ResampleHostTable> r_tab[vad::kMaxPumpRates];    // their tables and streaming rules (host)
    vad::PumpRates r_dev{};                      // ... and the engine's shared device images, as the kernel takes them
    int r_A = 0, r_hld = 0;                      // input samples a row holds at most (one chunk at the largest rate, rounded up to 8); pitch of d_hist
    // a resample slot / landing buffer: [rtab bytes: the row table, 32 bytes a row, ending where the flags start][hdr bytes: present[streams]]
    // [streams][r_A] int16
    size_t rtab = 0, res_bytes = 0;
    uint8_t *h_res = nullptr;                    // [R] resample slots, page-locked
    uint8_t *d_res = nullptr;                    // [NB] where a resampled tick's copy lands
    float *d_fbatch = nullptr;                   // [streams][N] fp32: the chunks a resampled tick steps (compute stream only: one buffer)
    float *d_fcarry = nullptr;                   // [streams][N] fp32: the outputs that wait for their chunk (in place)
    int16_t *d_hist = nullptr;                   // [streams][r_hld] the last H input samples of every bound stream, zero before its first
    std::vector<int8_t> r_rate;                  // [streams] the rate index a stream is bound to, -1: none (host bookkeeping, like held)
    std::vector<long> r_g, r_m;                  // [streams] inputs received / outputs emitted, both less the same whole periods
    std::vector<int32_t> r_pend;                 // [streams] fp32 outputs pending, 0 ... N - 1
    long n_bound = 0;                            // streams with r_rate[b] >= 0: the other routes look for them only while this is not 0
    struct Res { int32_t stream, pend; int8_t rate; long g, m; };
    std::vector<Res> r_new;                      // what each listed stream carries after the tick
    // snapshot / restore (vad_pump_export_streams / vad_pump_import_streams; allocated by the first of them, none of it touched by a tick)
    int32_t *h_snap_tab = nullptr;               // [streams] x {slot, part, pending, record}: page-locked, mapped -- the kernels read it in place
                                                 // (room for 2 x 4 words a stream: a version 2 entry goes on with {fp32 pending, H, bound, 0})
    int32_t *d_snap_tab = nullptr;               // device alias of h_snap_tab
    vad::SnapPart *d_snap_parts = nullptr;       // [parts] each part's state block and first slot
    uint8_t *d_snap = nullptr;                   // the packed records on the device: what the one copy of a call carries
    size_t snap_cap = 0;                         // ... its bytes
    // the tape in snapshots (vad_pump_export_streams_v3, and an import of a version 3 blob into a pump with a tape; allocated by the first
    // such call that moves a run, none of it touched by a tick or by the version 1 / 2 calls)
    vad::SnapRun *h_snap_runs = nullptr;         // [streams] the runs of a call: page-locked, mapped -- the kernels read it in place
    vad::SnapRun *d_snap_runs = nullptr;         // device alias of h_snap_runs
    uint8_t *d_snap_tape = nullptr;              // the packed runs on the device: what the one tape copy of a call carries
    size_t snap_tape_cap = 0;                    // ... its bytes
    // the tape (vad_pump_set_tape / vad_pump_set_tape_f32; tape_chunks == 0: not enabled, none of this is allocated and no tick launches
    // anything for it)
    int tape_chunks = 0;                         // chunks of a stream's ring
    int tape_elem = 0;                           // bytes of its element: 2 (int16), 4 (float: what the net read, also on a resampled tick); 0: no tape
    void *d_tape = nullptr;                      // [streams][tape_chunks][N] the chunks every stream was stepped on, chunk k in slot k % tape_chunks
    int64_t *d_tape_clock = nullptr;             // [streams][2] {count, floor}: written by tape_rows_kernel, open and import, on the compute stream
    std::vector<int64_t> tape_clock;             // [streams][2] what the last synchronising call read of it
    vad::TapeRequest *h_tape_req = nullptr, *d_tape_req = nullptr;      // the requests of a fetch: page-locked, and on the device
    size_t tape_req_cap = 0;                     // ... their number
    uint8_t *d_tape_out = nullptr, *h_tape_out = nullptr;               // a fetch into host memory: the packed samples on the device, and page-locked
    size_t tape_out_cap = 0;                     // ... their bytes
    bool poisoned = false;                      // a tick failed half-way: the carried state is no longer what any caller expects
    std::string err;

    int32_t *slot_pos(int r) const { return reinterpret_cast<int32_t *>(h_ring + (size_t)r * slot_bytes + htab); }
    uint8_t *slot_present(int r) const { return h_ring + (size_t)r * slot_bytes + htab + hpos; }
    int16_t *slot_pcm(int r) const { return reinterpret_cast<int16_t *>(h_ring + (size_t)r * slot_bytes + htab + hpos + hdr); }
    uint8_t *wide_present(int r) const { return h_wide + (size_t)r * wide_bytes + wtab; }
    float *step_probs(int r, int j) const {      // host side; the device aliases have the same layout
        return j == 0 ? h_prob + (size_t)r * streams : h_prob_more + ((size_t)r * (max_burst - 1) + (j - 1)) * streams;
    }
    uint8_t *res_present(int r) const { return h_res + (size_t)r * res_bytes + rtab; }
    void drop_held(int b) {
        n_held -= held[b] > 0;
        held[b] = 0;
    }
    bool bound(int b) const { return n_bound > 0 && r_rate[b] >= 0; }
    void unbind(int b) {                         // (host side; the device history is zeroed by the caller, in compute-stream order)
        if (!n_rates) return;
        n_bound -= r_rate[b] >= 0;
        r_rate[b] = -1;
        r_g[b] = r_m[b] = 0;
        r_pend[b] = 0;
    }
};

namespace {

int pfail(vad_pump *p, int code, const std::string &msg) {
    if (p) p->err = msg;
    return code;
}
#define PUMP_TRY(p, expr)                                                                               \
    do {                                                                                                \
        const hipError_t rc_ = (expr);                                                                  \
        if (rc_ != hipSuccess) return pfail(p, VAD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(rc_)); \
    } while (0)

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void cpu_relax() {
#if defined(__x86_64__)
    _mm_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

// dst <- src, `bytes` a multiple of 16, both 16-byte aligned on the destination side: streaming stores where the ISA has them (the
// data is bound for the DMA engine, not for this core's cache)
#if defined(__x86_64__)
__attribute__((target("avx2"))) inline void stream_copy_avx2(void *dst, const void *src, size_t bytes) {
    const __m256i *s = static_cast<const __m256i *>(src);
    __m256i *d = static_cast<__m256i *>(dst);
    for (size_t i = 0; i < bytes / 32; ++i) _mm256_stream_si256(d + i, _mm256_loadu_si256(s + i));
}
inline bool have_avx2() {
    static const bool v = __builtin_cpu_supports("avx2") && !std::getenv("SILERO_VAD_AMD_PUMP_SSE2");     // (A/B knob)
    return v;
}
inline bool want_prefetch() {
    static const bool v = !std::getenv("SILERO_VAD_AMD_PUMP_NO_PREFETCH");                                    // (A/B knob)
    return v;
}
#endif
// `next`: where the caller will read from next (the following stream's row, tens of KB away: no hardware prefetcher follows that) --
// its lines are requested while this row is being written
inline void stream_copy(void *dst, const void *src, size_t bytes, const void *next = nullptr) {
#if defined(__x86_64__)
    if (next && want_prefetch())
        for (size_t o = 0; o < bytes; o += 64) _mm_prefetch(static_cast<const char *>(next) + o, _MM_HINT_NTA);
    if (have_avx2() && bytes % 32 == 0 && (reinterpret_cast<size_t>(dst) & 31) == 0) return stream_copy_avx2(dst, src, bytes);
    const __m128i *s = static_cast<const __m128i *>(src);
    __m128i *d = static_cast<__m128i *>(dst);
    for (size_t i = 0; i < bytes / 16; ++i) _mm_stream_si128(d + i, _mm_loadu_si128(s + i));
#else
    (void)next;
    std::memcpy(dst, src, bytes);
#endif
}
inline void stream_fence() {
#if defined(__x86_64__)
    _mm_sfence();
#else
    std::atomic_thread_fence(std::memory_order_release);
#endif
}

// An event count: waiters spin for a bounded time on their own condition, then sleep in the kernel until somebody signals.  signal()
// is one atomic increment, plus a futex wake only if somebody sleeps.
struct Gate {
    std::atomic<uint32_t> seq{0};
    std::atomic<int> sleepers{0};
    static double spin_ms() {
        static const double v = [] {
            const char *s = std::getenv("SILERO_VAD_AMD_PUMP_SPIN_US");                                       // (A/B knob)
            return s ? std::atof(s) * 1e-3 : 0.020;
        }();
        return v;
    }

    template <class Cond>
    void wait(Cond cond) {
        const double t0 = now_ms(), limit = spin_ms();
        for (int i = 0;; ++i) {
            if (cond()) return;
            cpu_relax();
            if ((i & 63) == 63 && now_ms() - t0 > limit) break;
        }
        for (;;) {
            sleepers.fetch_add(1, std::memory_order_seq_cst);
            const uint32_t s = seq.load(std::memory_order_seq_cst);
            if (cond()) {
                sleepers.fetch_sub(1, std::memory_order_seq_cst);
                return;
            }
            // (a signal between the load of `seq` and here changes the word: the call returns at once)
            syscall(SYS_futex, reinterpret_cast<uint32_t *>(&seq), FUTEX_WAIT_PRIVATE, s, nullptr, nullptr, 0);
            sleepers.fetch_sub(1, std::memory_order_seq_cst);
        }
    }
    void signal() {
        seq.fetch_add(1, std::memory_order_seq_cst);
        if (sleepers.load(std::memory_order_seq_cst) > 0)
            syscall(SYS_futex, reinterpret_cast<uint32_t *>(&seq), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
    }
};

// host side of open / close: applied when the tick they were issued before is the next to retire (or at once if nothing is in flight)
void apply_ops(vad_pump *p) {
    while (!p->pending.empty() && p->pending.front().at_tick <= p->retired) {
        const vad_pump::Op op = p->pending.front();
        p->pending.pop_front();
        if (op.open) {
            p->active[op.stream] = 1;
            p->triggered[op.stream] = 0;
            p->temp_end[op.stream] = 0;
            p->current[op.stream] = 0;
            p->src_pos[op.stream] = 0;
        } else {
            p->active[op.stream] = 0;
        }
    }
}

}  // namespace

extern "C" {

void vad_pump_params_default(vad_pump_params *p, int sampling_rate, int streams) {
    if (!p) return;
    p->sampling_rate = sampling_rate;
    p->streams = streams;
    p->parts = 0;
    p->ring_slots = 0;
    p->threshold = 0.5;
    p->min_silence_duration_ms = 100;
    p->speech_pad_ms = 30;
}

const char *vad_pump_last_error(const vad_pump *p) { return p ? p->err.c_str() : "null pump"; }

void vad_pump_destroy(vad_pump *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    for (hipStream_t cs : p->copy)
        if (cs) (void)hipStreamSynchronize(cs);
    if (p->compute) (void)hipStreamSynchronize(p->compute);
    for (int b = 0; b < vad_pump::NB; ++b) {
        for (hipEvent_t ev : p->h2d_done[b]) (void)hipEventDestroy(ev);
        if (p->batch_free[b]) (void)hipEventDestroy(p->batch_free[b]);
    }
    for (int b = 0; b < 2; ++b)
        if (p->d_ctx[b]) (void)hipFree(p->d_ctx[b]);
    for (hipEvent_t ev : p->tick_done) (void)hipEventDestroy(ev);
    for (float *s : p->d_state) (void)hipFree(s);
    if (p->d_batch) (void)hipFree(p->d_batch);
    if (p->d_compact) (void)hipFree(p->d_compact);
    if (p->d_carry) (void)hipFree(p->d_carry);
    if (p->d_more) (void)hipFree(p->d_more);
    if (p->d_more_flags) (void)hipFree(p->d_more_flags);
    if (p->h_prob_more) (void)hipHostFree(p->h_prob_more);
    if (p->d_wide) (void)hipFree(p->d_wide);
    if (p->h_wide) (void)hipHostFree(p->h_wide);
    if (p->d_res) (void)hipFree(p->d_res);
    if (p->h_res) (void)hipHostFree(p->h_res);
    if (p->d_fbatch) (void)hipFree(p->d_fbatch);
    if (p->d_fcarry) (void)hipFree(p->d_fcarry);
    if (p->d_hist) (void)hipFree(p->d_hist);
    if (p->d_snap) (void)hipFree(p->d_snap);
    if (p->d_snap_parts) (void)hipFree(p->d_snap_parts);
    if (p->h_snap_tab) (void)hipHostFree(p->h_snap_tab);
    if (p->d_snap_tape) (void)hipFree(p->d_snap_tape);
    if (p->h_snap_runs) (void)hipHostFree(p->h_snap_runs);
    if (p->d_tape) (void)hipFree(p->d_tape);
    if (p->d_tape_clock) (void)hipFree(p->d_tape_clock);
    if (p->d_tape_req) (void)hipFree(p->d_tape_req);
    if (p->h_tape_req) (void)hipHostFree(p->h_tape_req);
    if (p->d_tape_out) (void)hipFree(p->d_tape_out);
    if (p->h_tape_out) (void)hipHostFree(p->h_tape_out);
    if (p->h_ring) (void)hipHostFree(p->h_ring);
    if (p->h_prob) (void)hipHostFree(p->h_prob);
    for (hipStream_t cs : p->copy)
        if (cs) (void)hipStreamDestroy(cs);
    if (p->compute) (void)hipStreamDestroy(p->compute);
    if (p->eng) vad_destroy(p->eng);
    delete p;
}

int vad_pump_create(vad_engine *e, const vad_pump_params *prm, vad_pump **out) {
    if (!out) return VAD_ERR_ARG;
    *out = nullptr;
    if (!e || !prm || prm->streams <= 0) return VAD_ERR_ARG;
    int N = 0, C = 0;
    if (vad_geometry(prm->sampling_rate, &N, &C) != VAD_OK) return VAD_ERR_SAMPLE_RATE;
    vad_pump *p = new (std::nothrow) vad_pump();
    if (!p) return VAD_ERR_ALLOC;
    auto bail = [&](int code) {
        vad_pump_destroy(p);
        return code;
    };
    p->sr = prm->sampling_rate;
    p->N = N;
    p->C = C;
    p->streams = prm->streams;
    p->R = prm->ring_slots > 0 ? std::max(2, prm->ring_slots) : 4;
    p->threshold = prm->threshold;
    p->min_silence = (double)p->sr * prm->min_silence_duration_ms / 1000.0;     // Python floats (utils_vad.py:494-498)
    p->pad = (double)p->sr * prm->speech_pad_ms / 1000.0;
    if (const char *v = std::getenv("SILERO_VAD_AMD_PUMP_BUFFERS")) p->nb = std::max(2, std::min(vad_pump::NB, std::atoi(v)));
    p->device = vad_device(e);
    if (p->device < 0 || vad_clone(e, &p->eng) != VAD_OK) return bail(VAD_ERR_NO_DEVICE);
    // the clone takes the caller's options with it; the pump steps through the product kernels whatever the caller's engine was set to
    // for its own A/B runs (impl=reference has no split-context step: every submit would fail)
    if (vad_set_option(p->eng, "impl", "mfma") != VAD_OK) return bail(VAD_ERR_OPTION);
    // parts of whole 16-stream tiles (a tile is the kernels' unit; rows of a part start 16-byte aligned)
    const int tiles = (p->streams + 15) / 16;
    const int parts = std::max(1, std::min(prm->parts > 0 ? prm->parts : 1, tiles));
    for (int k = 0; k < parts; ++k) {
        const int a = std::min(p->streams, (int)((long)tiles * k / parts) * 16), b = std::min(p->streams, (int)((long)tiles * (k + 1) / parts) * 16);
        if (b > a) {
            p->lo.push_back(a);
            p->hi.push_back(b);
        }
    }
    p->parts = (int)p->lo.size();
    if (hipSetDevice(p->device) != hipSuccess) return bail(VAD_ERR_HIP);
    const size_t S = (size_t)p->streams;
    p->hdr = (S + 4095) / 4096 * 4096;
    p->hpos = (S * sizeof(int32_t) + 4095) / 4096 * 4096;
    p->htab = (S * 4 * sizeof(int32_t) + 4095) / 4096 * 4096 - p->hpos;
    p->slot_bytes = p->htab + p->hpos + p->hdr + S * N * sizeof(int16_t);
    if (hipHostMalloc((void **)&p->h_ring, (size_t)p->R * p->slot_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&p->h_prob, (size_t)p->R * S * sizeof(float), hipHostMallocMapped) != hipSuccess)
        return bail(VAD_ERR_ALLOC);
    std::memset(p->h_ring, 0, (size_t)p->R * p->slot_bytes);
    for (int r = 0; r < p->R; ++r) std::memset(p->slot_present(r), 1, S);
    std::memset(p->h_prob, 0, (size_t)p->R * S * sizeof(float));
    void *dv = nullptr;
    if (hipHostGetDevicePointer(&dv, p->h_prob, 0) != hipSuccess || !dv) return bail(VAD_ERR_HIP);
    p->d_prob = static_cast<float *>(dv);
    if (hipMalloc((void **)&p->d_batch, vad_pump::NB * p->slot_bytes) != hipSuccess ||
        hipMalloc((void **)&p->d_compact, vad_pump::NB * p->slot_bytes) != hipSuccess ||
        hipMalloc((void **)&p->d_carry, S * N * sizeof(int16_t)) != hipSuccess)
        return bail(VAD_ERR_ALLOC);
    // (compact ticks fill only the delivering streams' rows; rows no tick has filled yet are computed too: let them be silence)
    if (hipMemset(p->d_batch, 0, vad_pump::NB * p->slot_bytes) != hipSuccess) return bail(VAD_ERR_HIP);
    for (int b = 0; b < 2; ++b) {
        if (hipMalloc((void **)&p->d_ctx[b], S * C * sizeof(float)) != hipSuccess) return bail(VAD_ERR_ALLOC);
        if (hipMemset(p->d_ctx[b], 0, S * C * sizeof(float)) != hipSuccess) return bail(VAD_ERR_HIP);
    }
    int maxB = 0;
    for (int k = 0; k < p->parts; ++k) {
        const size_t bytes = (size_t)2 * (p->hi[k] - p->lo[k]) * 128 * sizeof(float);
        float *st = nullptr;
        if (hipMalloc((void **)&st, bytes) != hipSuccess) return bail(VAD_ERR_ALLOC);
        p->d_state.push_back(st);
        if (hipMemset(st, 0, bytes) != hipSuccess) return bail(VAD_ERR_HIP);
        maxB = std::max(maxB, p->hi[k] - p->lo[k]);
    }
    if (hipStreamCreateWithFlags(&p->copy[0], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&p->copy[1], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&p->compute, hipStreamNonBlocking) != hipSuccess)
        return bail(VAD_ERR_HIP);
    auto mk = [&](hipEvent_t *ev) { return hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess; };
    for (int b = 0; b < vad_pump::NB; ++b) {
        p->h2d_done[b].resize(p->parts);
        for (auto &ev : p->h2d_done[b])
            if (!mk(&ev)) return bail(VAD_ERR_HIP);
        if (!mk(&p->batch_free[b])) return bail(VAD_ERR_HIP);
    }
    p->tick_done.resize(p->R);
    // a process with CPUs to spare lets hipEventSynchronize spin on the tick's event (lowest latency); one with fewer than four (one of
    // eight ranks under a 16-CPU quota) sleeps on the interrupt instead: the CPU the spin would burn is the source thread's
    const bool blocking = vad::default_host_threads(256) < 4;
    for (auto &ev : p->tick_done)
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming | (blocking ? hipEventBlockingSync : 0)) != hipSuccess) return bail(VAD_ERR_HIP);
    if (vad_reserve(p->eng, p->sr, maxB, 1) != VAD_OK) return bail(VAD_ERR_ALLOC);
    if (hipDeviceSynchronize() != hipSuccess) return bail(VAD_ERR_HIP);
    p->slot_busy.assign(p->R, 0);
    p->slot_steps.assign(p->R, 1);
    p->active.assign(S, 1);
    p->feed_mask.assign(S, 1);
    p->triggered.assign(S, 0);
    p->temp_end.assign(S, 0);
    p->current.assign(S, 0);
    p->src_pos.assign(S, 0);
    p->held.assign(S, 0);
    p->seen.assign(S, 0);
    *out = p;
    return VAD_OK;
}

int vad_pump_geometry(const vad_pump *p, int *streams, int *chunk, int *ring_slots, int *parts) {
    if (!p) return VAD_ERR_ARG;
    if (streams) *streams = p->streams;
    if (chunk) *chunk = p->N;
    if (ring_slots) *ring_slots = p->R;
    if (parts) *parts = p->parts;
    return VAD_OK;
}

int16_t *vad_pump_slot(vad_pump *p, int r) { return (p && r >= 0 && r < p->R) ? p->slot_pcm(r) : nullptr; }

uint8_t *vad_pump_present(vad_pump *p, int r) { return (p && r >= 0 && r < p->R) ? p->slot_present(r) : nullptr; }

const float *vad_pump_probs(const vad_pump *p, int r) {
    return (p && r >= 0 && r < p->R) ? p->h_prob + (size_t)r * p->streams : nullptr;
}

}  // extern "C"

namespace {

// a packet tick's rows (vad_pump_submit_packets; vad_pump_submit_coded_packets: `coded`, offsets in bytes, codec per row or null)
struct Packets {
    const int32_t *stream, *off, *len;
    bool coded = false;
    const uint8_t *codec = nullptr;
    bool burst = false;                          // vad_pump_submit_burst: a stream may have several rows, a row may be longer than N
    bool wide = false;                           // vad_pump_submit_wide_packets: int16 rows of the WIDE slot, sampled at step x 16 kHz
    const uint8_t *step = nullptr;               // ... the step per row, or null (every row at max_step)
    bool res = false;                            // vad_pump_submit_resampled_packets: int16 rows of the RESAMPLE slot, at rates[rate of row]
    const uint8_t *rate = nullptr;               // ... the rate index per row, or null (every row at rate 0)
};
const char *const kCodecWhy[2] = {" is none of VAD_PCM_S16 / VAD_PCM_ULAW / VAD_PCM_ALAW (VAD_PCM_DVI4 rows are not enabled on this pump: vad_pump_set_adpcm)",
                                   " is none of VAD_PCM_S16 / VAD_PCM_ULAW / VAD_PCM_ALAW / VAD_PCM_DVI4"};
const char *const kOddWhy = "a DVI4 row of an odd length (its codes come two a byte)";
// the bytes a payload row of `len` samples takes in the slot: 2 a sample, 1 a sample (G.711), or a 4-byte header and 2 samples a byte
inline long row_bytes(int codec, long len) { return codec == VAD_PCM_S16 ? 2 * len : codec == VAD_PCM_DVI4 ? 4 + len / 2 : len; }
const char *const kBoundWhy = "a stream that is bound to a resampled rate (vad_pump_submit_resampled_packets) until vad_pump_open / vad_pump_close";

// Validate a packet tick's rows and write its row table (ending where slot r's flags start) and its flags (the streams that complete
// a chunk).  -> the bytes of the slot's sample area the copy has to carry, or < 0 (VAD_ERR_ARG, p->err says why; nothing queued).
// *g711: a row is not int16 -- the table then holds byte offsets and each row's codec in the high bits of its length, for
// assemble_coded_packets; otherwise it holds sample offsets, for assemble_packets, whichever entry point was called.  *adpcm: one of
// those rows is DVI4 (an even length, 4 + len / 2 bytes) -- the same table, for assemble_adpcm_packets.
// A SILENT row (offset VAD_ROW_SILENT: len samples of digital silence, no bytes in the slot) keeps the marker in the table's offset
// column, is S16 whatever codec_of_row says (its entry is not looked at, it does not make the tick a G.711 tick), passes neither the
// alignment nor the fits-the-area check and does not count towards the bytes the copy carries; everything else applies to it.
long build_packets(vad_pump *p, int r, const Packets &pk, long n_rows, bool *g711, bool *adpcm) {
    const long S = p->streams, N = p->N;
    const char *fn = pk.coded ? "vad_pump_submit_coded_packets: " : "vad_pump_submit_packets: ";
    if (n_rows < 0 || n_rows > S || (n_rows > 0 && (!pk.stream || !pk.off || !pk.len)))
        return pfail(p, VAD_ERR_ARG, std::string(fn) + "bad row list"), -1;
    *g711 = *adpcm = false;
    for (long i = 0; pk.codec && i < n_rows; ++i) {
        if (pk.off[i] == VAD_ROW_SILENT) continue;
        if (pk.codec[i] > (p->adpcm ? VAD_PCM_DVI4 : VAD_PCM_ALAW))
            return pfail(p, VAD_ERR_ARG, std::string(fn) + "row " + std::to_string(i) + ": codec " + std::to_string(pk.codec[i]) + kCodecWhy[p->adpcm]), -1;
        *g711 |= pk.codec[i] != VAD_PCM_S16;
        *adpcm |= pk.codec[i] == VAD_PCM_DVI4;
    }
    uint8_t *fl = p->slot_present(r);
    int32_t *tab = reinterpret_cast<int32_t *>(fl) - 4 * n_rows;
    std::memset(fl, 0, (size_t)S);
    long end = 0, i = 0;
    const char *why = nullptr;
    for (; i < n_rows && !why; ++i) {
        const int32_t b = pk.stream[i], off = pk.off[i], len = pk.len[i];
        const bool silent = off == VAD_ROW_SILENT;
        const int codec = pk.codec && !silent ? pk.codec[i] : VAD_PCM_S16;
        const long at = pk.coded ? off : 2L * off, bytes = row_bytes(codec, len);      // the row, in bytes
        if (b < 0 || b >= S || p->seen[b]) why = "a stream out of range, or listed twice in one tick";
        else if (p->bound(b)) why = kBoundWhy;
        else if (len < 1 || len > N) why = "a packet length out of 1 ... N (a longer packet goes in over two ticks)";
        else if (codec == VAD_PCM_DVI4 && len % 2) why = kOddWhy;
        else if (!silent && (at < 0 || at % 16 || at + bytes > S * N * 2))
            why = pk.coded ? "a packet byte offset that is not a multiple of 16, or a row that runs past the slot"
                           : "a packet offset that is not a multiple of 8 samples, or runs past the slot";
        else {
            p->seen[b] = 1;
            const int32_t c = p->held[b];
            tab[4 * i] = b, tab[4 * i + 1] = silent ? VAD_ROW_SILENT : (int32_t)(*g711 ? at : at / 2), tab[4 * i + 2] = len | codec << vad::kCodecShift, tab[4 * i + 3] = c;
            fl[b] = c + len >= N;
            if (!silent) end = std::max(end, (at + bytes + 15) / 16 * 16);
        }
    }
    for (long k = 0; k < i; ++k)                 // (only valid streams were marked)
        if (pk.stream[k] >= 0 && pk.stream[k] < S) p->seen[pk.stream[k]] = 0;
    if (why) {
        std::memset(fl, 0, (size_t)S);
        return pfail(p, VAD_ERR_ARG, std::string(fn) + why), -1;
    }
    return end;
}

// The same for a burst tick (vad_pump_submit_burst).  The row table is written GROUPED BY STREAM (a counting sort over the tick's rows:
// streams by first appearance, a stream's rows in arrival order): {stream, byte offset, len | codec, w}, w = pending before | k <<
// kCodecShift on a stream's first row, -1 on its others -- assemble_burst's work unit is the stream.  The flag byte of a listed stream
// holds k, the chunks it completes (0 ... max_burst).  *steps = max(1, largest k).  The pending counts are NOT touched: p->b_new holds
// them for the caller to apply once the tick is queued.  A SILENT row (offset VAD_ROW_SILENT) is a row of any length >= 1 like another:
// S16 in the table whatever its codec entry says, no offset checks, no bytes of the copy.
long build_burst(vad_pump *p, int r, const Packets &pk, long n_rows, int *steps, bool *adpcm) {
    const long S = p->streams, N = p->N, M = p->max_burst;
    const std::string fn = "vad_pump_submit_burst: ";
    if (M < 1) return pfail(p, VAD_ERR_ARG, fn + "bursts are not enabled on this pump (vad_pump_set_burst)"), -1;
    if (n_rows < 0 || n_rows > S || (n_rows > 0 && (!pk.stream || !pk.off || !pk.len)))
        return pfail(p, VAD_ERR_ARG, fn + "bad row list (a tick holds at most `streams` rows)"), -1;
    *adpcm = false;
    for (long i = 0; pk.codec && i < n_rows; ++i) {
        if (pk.off[i] == VAD_ROW_SILENT) continue;
        if (pk.codec[i] > (p->adpcm ? VAD_PCM_DVI4 : VAD_PCM_ALAW))
            return pfail(p, VAD_ERR_ARG, fn + "row " + std::to_string(i) + ": codec " + std::to_string(pk.codec[i]) + kCodecWhy[p->adpcm]), -1;
        *adpcm |= pk.codec[i] == VAD_PCM_DVI4;
    }
    p->b_touched.clear();
    p->b_new.clear();
    long end = 0;
    const char *why = nullptr;
    for (long i = 0; i < n_rows && !why; ++i) {
        const int32_t b = pk.stream[i];
        const long at = pk.off[i], len = pk.len[i];
        const bool silent = at == VAD_ROW_SILENT;
        const int codec = pk.codec && !silent ? pk.codec[i] : VAD_PCM_S16;
        const long bytes = row_bytes(codec, len);
        if (b < 0 || b >= S) why = "a stream out of range";
        else if (p->bound(b)) why = kBoundWhy;
        else if (len < 1) why = "a row length below 1";
        else if (codec == VAD_PCM_DVI4 && len % 2) why = kOddWhy;
        else if (!silent && (at < 0 || at % 16 || at + bytes > S * N * 2)) why = "a row byte offset that is not a multiple of 16, or a row that runs past the slot";
        else {
            if (p->b_cnt[b]++ == 0) p->b_touched.push_back(b);
            if (p->held[b] + p->b_len[b] + len >= (M + 1) * N) why = "a stream would complete more than max_chunks chunks in one tick";
            else p->b_len[b] += (int32_t)len;
            if (!silent) end = std::max(end, (at + bytes + 15) / 16 * 16);
        }
    }
    if (why) {
        for (const int32_t b : p->b_touched) p->b_cnt[b] = p->b_len[b] = 0;
        return pfail(p, VAD_ERR_ARG, fn + why), -1;
    }
    int32_t row = 0, kmax = 0;
    for (const int32_t b : p->b_touched) {
        p->b_pos[b] = row;
        row += p->b_cnt[b];
    }
    uint8_t *fl = p->slot_present(r);
    int32_t *tab = reinterpret_cast<int32_t *>(fl) - 4 * n_rows;
    std::memset(fl, 0, (size_t)S);
    for (long i = 0; i < n_rows; ++i) {
        const int32_t b = pk.stream[i], c = p->held[b], k = (int32_t)((c + p->b_len[b]) / N);
        const bool first = p->b_cnt[b] != 0;                 // (the row count has done its work: positions are assigned)
        p->b_cnt[b] = 0;
        int32_t *e = tab + 4 * (size_t)p->b_pos[b]++;
        e[0] = b, e[1] = pk.off[i], e[2] = pk.len[i] | (pk.codec && pk.off[i] != VAD_ROW_SILENT ? pk.codec[i] : VAD_PCM_S16) << vad::kCodecShift;
        e[3] = first ? c | k << vad::kCodecShift : -1;
    }
    for (const int32_t b : p->b_touched) {
        const int32_t total = p->held[b] + p->b_len[b], k = (int32_t)(total / N);
        fl[b] = (uint8_t)k;
        kmax = std::max(kmax, k);
        p->b_new.push_back(vad_pump::Held{b, (int32_t)(total - k * N)});
        p->b_len[b] = 0;
    }
    *steps = std::max(1, kmax);
    return end;
}

// The same for a wide tick (vad_pump_submit_wide_packets): the table and the flags go into WIDE slot r, table[i] = {stream, byte offset,
// len | step << kCodecShift | first kept sample << kCombShift, pending before}.  A stream completes a chunk when its pending samples plus
// the row's KEPT samples reach N.  Neither the pending counts nor the phases are touched: p->w_new holds them for the caller to apply
// once the tick is queued.  A SILENT row (offset VAD_ROW_SILENT) stands for len input samples of silence at its step: the phase advances
// by len and comb_kept zeros are appended, as for a payload row; no offset checks, no bytes of the copy.
long build_wide(vad_pump *p, int r, const Packets &pk, long n_rows) {
    const long S = p->streams, N = p->N, M = p->max_step;
    const std::string fn = "vad_pump_submit_wide_packets: ";
    if (M < 2) return pfail(p, VAD_ERR_ARG, fn + "wideband is not enabled on this pump (vad_pump_set_wideband)"), -1;
    if (n_rows < 0 || n_rows > S || (n_rows > 0 && (!pk.stream || !pk.off || !pk.len)))
        return pfail(p, VAD_ERR_ARG, fn + "bad row list (a tick holds at most `streams` rows)"), -1;
    uint8_t *fl = p->wide_present(r);
    int32_t *tab = reinterpret_cast<int32_t *>(fl) - 4 * n_rows;
    std::memset(fl, 0, (size_t)S);
    p->w_new.clear();
    const long area = S * N * M * 2;             // bytes of the wide slot's sample area
    long end = 0, i = 0;
    const char *why = nullptr;
    for (; i < n_rows && !why; ++i) {
        const int32_t b = pk.stream[i];
        const long at = pk.off[i], len = pk.len[i], step = pk.step ? pk.step[i] : M;
        const bool silent = at == VAD_ROW_SILENT;
        if (step < 1 || step > M) why = "a step out of 1 ... max_step";
        else if (b < 0 || b >= S || p->seen[b]) why = "a stream out of range, or listed twice in one tick";
        else if (p->bound(b)) why = kBoundWhy;
        else if (len < 1 || len > step * N) why = "a row length out of 1 ... step * N (a longer row goes in over two ticks)";
        else if (!silent && (at < 0 || at % 16 || at + 2 * len > area)) why = "a row byte offset that is not a multiple of 16, or a row that runs past the wide slot";
        else {
            p->seen[b] = 1;
            const int32_t c = p->held[b], phase = step == p->w_step[b] ? p->w_phase[b] : 0;      // (another step: the comb starts anew)
            const int32_t k0 = vad::comb_first((int)step, phase), total = c + vad::comb_kept((int)step, k0, (int)len);
            tab[4 * i] = b, tab[4 * i + 1] = (int32_t)at, tab[4 * i + 2] = (int32_t)(len | step << vad::kCodecShift | (long)k0 << vad::kCombShift), tab[4 * i + 3] = c;
            fl[b] = total >= N;
            p->w_new.push_back(vad_pump::Comb{b, (int32_t)(total >= N ? total - N : total), (uint8_t)step, (uint8_t)((phase + len) % step)});
            if (!silent) end = std::max(end, (at + 2 * len + 15) / 16 * 16);
        }
    }
    for (long k = 0; k < i; ++k)                 // (only valid streams were marked)
        if (pk.stream[k] >= 0 && pk.stream[k] < S) p->seen[pk.stream[k]] = 0;
    if (why) {
        std::memset(fl, 0, (size_t)S);
        return pfail(p, VAD_ERR_ARG, fn + why), -1;
    }
    return end;
}

// The same for a resampled tick (vad_pump_submit_resampled_packets): the table (kResampleRowWords int32 a row, device_api.hpp) and the
// flags go into RESAMPLE slot r.  Per row the host runs the streaming rule: with g inputs received and m outputs emitted (both less the
// same whole periods) a row of len samples emits outputs m ... ready(g + len) - 1; the first of them is phase j0 = m % N of period
// q0 = m / N, and input position p of the stream lies at p - (g - H) of the wave's staged history ++ row, so output i reads from
// base + dq O + first[j], base = q0 O - W - g + H.  A stream completes a chunk when its fp32 pending outputs plus the row's reach the
// chunk.  Nothing of the bookkeeping is touched: p->r_new holds it for the caller to apply once the tick is queued.  A SILENT row
// stands for len input samples of silence: zeros enter the filter; no offset checks, no bytes of the copy.
long build_resampled(vad_pump *p, int r, const Packets &pk, long n_rows) {
    const long S = p->streams, N = p->N, A = p->r_A;
    const std::string fn = "vad_pump_submit_resampled_packets: ";
    if (!p->n_rates) return pfail(p, VAD_ERR_ARG, fn + "resampled rows are not enabled on this pump (vad_pump_set_resample)"), -1;
    if (n_rows < 0 || n_rows > S || (n_rows > 0 && (!pk.stream || !pk.off || !pk.len)))
        return pfail(p, VAD_ERR_ARG, fn + "bad row list (a tick holds at most `streams` rows)"), -1;
    uint8_t *fl = p->res_present(r);
    int32_t *tab = reinterpret_cast<int32_t *>(fl) - vad::kResampleRowWords * n_rows;
    std::memset(fl, 0, (size_t)S);
    p->r_new.clear();
    const long area = S * A * 2;                 // bytes of the resample slot's sample area
    long end = 0, i = 0;
    const char *why = nullptr;
    for (; i < n_rows && !why; ++i) {
        const int32_t b = pk.stream[i];
        const long at = pk.off[i], len = pk.len[i], k = pk.rate ? pk.rate[i] : 0;
        const bool silent = at == VAD_ROW_SILENT;
        if (k >= p->n_rates) why = "a rate index out of 0 ... n_rates - 1";
        else if (b < 0 || b >= S || p->seen[b]) why = "a stream out of range, or listed twice in one tick";
        else if (p->r_rate[b] >= 0 && p->r_rate[b] != k) why = "a row at another rate than the one the stream is bound to (vad_pump_open unbinds)";
        else if (p->held[b] > 0) why = "a stream with int16 samples pending from another packet route";
        else if (len < 1 || len > A) why = "a row length out of 1 ... the slot's samples per stream (a longer row goes in over two ticks)";
        else if (!silent && (at < 0 || at % 16 || at + 2 * len > area)) why = "a row byte offset that is not a multiple of 16, or a row that runs past the resample slot";
        else {
            const vad::ResampleHostTable &t = *p->r_tab[k];
            const bool is_bound = p->r_rate[b] >= 0;
            const long g = is_bound ? p->r_g[b] : 0, m = is_bound ? p->r_m[b] : 0, c = is_bound ? p->r_pend[b] : 0;
            const long m1 = vad::resample_stream_ready(t, g + len), n_out = m1 - m, total = c + n_out;
            if (total >= 2 * N) {
                why = "a row that would complete more than one chunk of its stream (submit it over two ticks)";
                break;
            }
            p->seen[b] = 1;
            const long O = t.g.O, Nr = t.g.N, q0 = m / Nr, j0 = m - q0 * Nr;
            int32_t *e = tab + vad::kResampleRowWords * i;
            e[0] = b, e[1] = (int32_t)at, e[2] = (int32_t)(len | k << vad::kResampleRateShift), e[3] = (int32_t)c;
            e[4] = (int32_t)(q0 * O - t.g.W - g + t.H), e[5] = (int32_t)j0, e[6] = (int32_t)n_out, e[7] = 0;
            fl[b] = total >= N;
            const long periods = m1 / Nr;       // complete at g + len: they leave both counters (the rule is periodic behind them)
            p->r_new.push_back(vad_pump::Res{b, (int32_t)(total >= N ? total - N : total), (int8_t)k, g + len - periods * O, m1 - periods * Nr});
            if (!silent) end = std::max(end, (at + 2 * len + 15) / 16 * 16);
        }
    }
    for (long k = 0; k < i && k < n_rows; ++k)   // (only valid streams were marked)
        if (pk.stream[k] >= 0 && pk.stream[k] < S) p->seen[pk.stream[k]] = 0;
    if (why) {
        std::memset(fl, 0, (size_t)S);
        return pfail(p, VAD_ERR_ARG, fn + why), -1;
    }
    return end;
}

// rows != nullptr: a compact tick whose rows lie in ARRIVAL order -- row i of the slot is the chunk of stream rows[i] (n_rows of them);
// flags and positions are built here.  rows == nullptr && compact: row i is the i-th stream (ascending) whose flag is set.
// pk != nullptr: a packet tick of n_rows rows (compact: its copy lands in the compact buffers, and masked).
int submit_tick(vad_pump *p, int r, const uint8_t *present, bool compact, const int32_t *rows = nullptr, long n_rows = 0,
                const Packets *pk = nullptr) {
    if (!p) return VAD_ERR_ARG;
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (r < 0 || r >= p->R) return pfail(p, VAD_ERR_ARG, "vad_pump_submit: no such ring slot");
    if (p->slot_busy[r]) return pfail(p, VAD_ERR_ARG, "vad_pump_submit: the slot's previous tick has not been retired (vad_pump_poll)");
    PUMP_TRY(p, hipSetDevice(p->device));
    const int buf = (int)(p->ticks % p->nb), pp = (int)(p->ticks & 1), cp = (int)(p->flips & 1);
    const size_t S = (size_t)p->streams, N = (size_t)p->N, C = (size_t)p->C;
    long pk_bytes = 0;                           // a packet tick: the bytes of the slot's sample area its copy carries
    bool g711 = false, adpcm = false;            // ... and it has a row that is not int16, a DVI4 row
    int steps = 1;                               // a burst tick: the masked steps it runs
    if (pk) {
        if ((pk_bytes = pk->res     ? build_resampled(p, r, *pk, n_rows)
                        : pk->wide  ? build_wide(p, r, *pk, n_rows)
                        : pk->burst ? build_burst(p, r, *pk, n_rows, &steps, &adpcm)
                                    : build_packets(p, r, *pk, n_rows, &g711, &adpcm)) < 0)
            return VAD_ERR_ARG;
        present = pk->res ? p->res_present(r) : pk->wide ? p->wide_present(r) : p->slot_present(r);      // (a wide / resampled tick's flags: copied to the slot's own row for vad_pump_poll)
    } else if (rows != nullptr || n_rows != 0) {
        if (!rows || n_rows < 0 || n_rows > (long)S) return pfail(p, VAD_ERR_ARG, "vad_pump_submit_rows: bad row list");
        uint8_t *fl = p->slot_present(r);
        int32_t *pos = p->slot_pos(r);
        std::memset(fl, 0, S);
        for (long i = 0; i < n_rows; ++i) {
            const int32_t b = rows[i];
            if (b < 0 || (size_t)b >= S || fl[b]) {          // (validated before anything is queued: the slot's flags are scratch until then)
                std::memset(fl, 0, S);
                return pfail(p, VAD_ERR_ARG, "vad_pump_submit_rows: a stream out of range, or listed twice in one tick");
            }
            fl[b] = 1;
            pos[b] = (int32_t)i;
        }
        present = fl;
    }
    const bool masked = present != nullptr;
    if (compact && !masked) return pfail(p, VAD_ERR_ARG, "vad_pump_submit_compact: a compact tick needs its flags");
    if (!pk && p->n_held > 0) {                  // a chunk may not overtake samples a stream has pending from its packets
        for (size_t b = 0; b < S; ++b)
            if (p->held[b] > 0 && (!masked || present[b]))
                return pfail(p, VAD_ERR_ARG, "vad_pump_submit: stream " + std::to_string(b) +
                                                 " has samples pending from packets; its next chunk must arrive as packets");
    }
    if (!pk && p->n_bound > 0) {                 // ... nor may a chunk enter a stream whose samples pass the resampler
        for (size_t b = 0; b < S; ++b)
            if (p->r_rate[b] >= 0 && (!masked || present[b]))
                return pfail(p, VAD_ERR_ARG, "vad_pump_submit: stream " + std::to_string(b) + 
                                                 " is bound to a resampled rate; until vad_pump_open / vad_pump_close its samples arrive as resampled rows");
    }
    if (masked && present != p->slot_present(r)) std::memcpy(p->slot_present(r), present, S);
    uint8_t *dbuf = p->d_batch + (size_t)buf * p->slot_bytes + p->htab;
    int16_t *batch = reinterpret_cast<int16_t *>(dbuf + p->hpos + p->hdr);
    const uint8_t *d_present = masked ? dbuf + p->hpos : nullptr;
    uint8_t *cbuf = nullptr;                     // compact tick: where its one copy lands
    size_t n_present = 0;
    if (compact) {
        cbuf = p->d_compact + (size_t)buf * p->slot_bytes + p->htab;
        d_present = cbuf + p->hpos;
        // the position table: row of the slot that holds stream b's chunk (the i-th delivering stream's chunk is row i)
        const uint8_t *fl = p->slot_present(r);
        int32_t *pos = p->slot_pos(r);
        if (pk && pk->res) {
            d_present = p->d_res + (size_t)buf * p->res_bytes + p->rtab;        // (its copy lands in the resample buffer, flags included)
        } else if (pk && pk->wide) {
            d_present = p->d_wide + (size_t)buf * p->wide_bytes + p->wtab;      // (its copy lands in the wide buffer, flags included)
        } else if (pk) {
            // (no position table: the row table written with the flags lies over it)
        } else if (rows != nullptr) {
            n_present = (size_t)n_rows;                  // (positions were written with the flags)
        } else {
            for (size_t b = 0; b < S; ++b) {
                pos[b] = (int32_t)n_present;
                n_present += fl[b] != 0;
            }
        }
    }
    const int16_t *src = p->slot_pcm(r);
    hipStream_t copy = p->copy[pp];
    // from the first queued operation on, a failure leaves the tick half-done: (h, c) of some parts advanced, the context ping-pong out
    // of step.  There is no retry that is right; the pump says so from then on.
    auto broken = [&](int code, const std::string &msg) {
        p->poisoned = true;
        return pfail(p, code, msg);
    };
#define TICK_TRY(expr)                                                                                  \
    do {                                                                                                \
        const hipError_t rc_ = (expr);                                                                  \
        if (rc_ != hipSuccess) return broken(VAD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(rc_)); \
    } while (0)
    // the copies may not overwrite the batch buffer before the kernels of two ticks ago have read it
    if (p->batch_used[buf]) TICK_TRY(hipStreamWaitEvent(copy, p->batch_free[buf], 0));
    if (pk) {
        // ONE copy: row table + flags + the packets; the assembly pass on the compute stream splices the completing streams' rows out
        // of their carries and their packets (the carry's previous users and the batch buffer's previous readers are earlier there)
        const size_t tab_bytes = (size_t)n_rows * (pk->res ? vad::kResampleRowWords : 4) * sizeof(int32_t);
        const uint8_t *h_fl = pk->res ? p->res_present(r) : pk->wide ? p->wide_present(r) : p->slot_present(r);      // the flags of the slot the rows lie in
        uint8_t *d_fl = pk->res    ? p->d_res + (size_t)buf * p->res_bytes + p->rtab                        // ... and of the buffer they land in
                        : pk->wide ? p->d_wide + (size_t)buf * p->wide_bytes + p->wtab
                                   : cbuf + p->hpos;
        TICK_TRY(hipMemcpyAsync(d_fl - tab_bytes, h_fl - tab_bytes, tab_bytes + p->hdr + pk_bytes, hipMemcpyHostToDevice, copy));
        TICK_TRY(hipEventRecord(p->h2d_done[buf][0], copy));
        TICK_TRY(hipStreamWaitEvent(p->compute, p->h2d_done[buf][0], 0));
        const int32_t *table = reinterpret_cast<const int32_t *>(d_fl - tab_bytes);
        if (pk->res) {                           // (the rows pass the filter on the way; the chunks are fp32, in the one fp32 batch)
            TICK_TRY(vad::launch_assemble_resampled_packets(table, n_rows, d_fl + p->hdr, p->r_dev, p->d_hist, p->r_hld, p->r_A, p->d_fcarry,
                                                            p->d_fbatch, p->N, p->compute));
        } else if (pk->wide) {                   // (the rows are decimated on the way; the carry holds 16 kHz samples)
            TICK_TRY(vad::launch_assemble_wide_packets(table, n_rows, d_fl + p->hdr, p->d_carry, batch, p->N, p->compute));
        } else if (pk->burst) {                  // (chunk 0 of every stream into `batch`, chunks 1 ... into d_more; flags_j = k > j)
            TICK_TRY(vad::launch_assemble_burst(table, n_rows, cbuf + p->hpos + p->hdr, p->d_carry, batch, p->d_more, p->max_burst, p->streams, p->N,
                                                adpcm, p->compute));
            TICK_TRY(vad::launch_burst_flags(d_present, p->d_more_flags, (long)p->hdr, steps, p->streams, p->compute));
        } else if (adpcm)                        // (a DVI4 row is decoded on the way, by two wave scans; only such ticks take this kernel)
            TICK_TRY(vad::launch_assemble_adpcm_packets(table, n_rows, cbuf + p->hpos + p->hdr, p->d_carry, batch, p->N, p->compute));
        else if (g711)                           // (G.711 rows are expanded on the way; an all-int16 tick takes the int16 kernel)
            TICK_TRY(vad::launch_assemble_coded_packets(table, n_rows, cbuf + p->hpos + p->hdr, p->d_carry, batch, p->N, p->compute));
        else
            TICK_TRY(vad::launch_assemble_packets(table, n_rows, reinterpret_cast<const int16_t *>(cbuf + p->hpos + p->hdr), p->d_carry, batch,
                                                  p->N, p->compute));
    } else if (compact) {
        // ONE copy whatever `parts` says: table + flags + the delivering streams' rows; the expansion pass on the compute stream puts
        // every row where the kernels read it (the batch buffer's previous readers are earlier on that stream)
        TICK_TRY(hipMemcpyAsync(cbuf, p->slot_pos(r), p->hpos + p->hdr + n_present * N * sizeof(int16_t), hipMemcpyHostToDevice, copy));
        TICK_TRY(hipEventRecord(p->h2d_done[buf][0], copy));
        TICK_TRY(hipStreamWaitEvent(p->compute, p->h2d_done[buf][0], 0));
        TICK_TRY(vad::launch_expand_rows(d_present, reinterpret_cast<const int32_t *>(cbuf), cbuf + p->hpos + p->hdr, batch,
                                         (long)(N * sizeof(int16_t)), p->streams, p->compute));
    }
    for (int k = 0; k < p->parts && !compact; ++k) {
        const size_t a = (size_t)p->lo[k], n = (size_t)(p->hi[k] - p->lo[k]);
        if (k == 0 && masked)        // the flags of ALL streams ride in front of part 0's audio: one copy (part 0 starts at stream 0)
            TICK_TRY(hipMemcpyAsync(dbuf + p->hpos, p->slot_present(r), p->hdr + n * N * sizeof(int16_t), hipMemcpyHostToDevice, copy));
        else
            TICK_TRY(hipMemcpyAsync(batch + a * N, src + a * N, n * N * sizeof(int16_t), hipMemcpyHostToDevice, copy));
        TICK_TRY(hipEventRecord(p->h2d_done[buf][k], copy));
    }
    for (int j = 0; j < steps; ++j) {            // (one step; a burst tick: sub-step j over the chunks j of the streams with k > j)
        const int16_t *rows_j = j == 0 ? batch : p->d_more + (size_t)(j - 1) * S * N;
        const uint8_t *flags_j = j == 0 ? d_present : p->d_more_flags + (size_t)(j - 1) * p->hdr;
        float *probs_j = j == 0 ? p->d_prob + (size_t)r * S : p->d_prob_more + ((size_t)r * (p->max_burst - 1) + (j - 1)) * S;
        const float *ctx_in = p->d_ctx[(cp + j) & 1];
        float *ctx_out = p->d_ctx[(cp + j + 1) & 1];
        for (int k = 0; k < p->parts; ++k) {
            const size_t a = (size_t)p->lo[k];
            const int n = p->hi[k] - p->lo[k];
            if (!compact) TICK_TRY(hipStreamWaitEvent(p->compute, p->h2d_done[buf][k], 0));
            if (k > 0 && masked && !compact) TICK_TRY(hipStreamWaitEvent(p->compute, p->h2d_done[buf][0], 0));     // (the flags came with part 0)
            const bool f32 = pk && pk->res;      // (a resampled tick steps the fp32 batch; everything else about the step is the same)
            const int rc = vad_step_present(p->eng, p->sr, n, f32 ? (const void *)(p->d_fbatch + a * N) : (const void *)(rows_j + a * N),
                                            f32 ? sizeof(float) : sizeof(int16_t), (long)N, ctx_in + a * C, ctx_out + a * C, p->d_state[k],
                                            probs_j + a, masked ? flags_j + a : nullptr, p->compute);
            if (rc != VAD_OK) return broken(rc, std::string("vad_step_present: ") + vad_last_error(p->eng));
        }
        // the tape: the rows this step read, of the streams it stepped (behind the last part: every h2d_done wait has been made)
        // (a resampled tick: its rows of the one fp32 batch, which nothing overwrites before the next resampled tick's assembly, later
        // on this stream)
        if (p->tape_elem == 2)
            TICK_TRY(vad::launch_tape_rows(rows_j, masked ? flags_j : nullptr, static_cast<int16_t *>(p->d_tape), p->d_tape_clock, p->tape_chunks,
                                           p->streams, p->N, p->compute));
        else if (p->tape_elem == 4 && pk && pk->res)
            TICK_TRY(vad::launch_tape_rows(p->d_fbatch, masked ? flags_j : nullptr, static_cast<float *>(p->d_tape), p->d_tape_clock, p->tape_chunks,
                                           p->streams, p->N, p->compute));
        else if (p->tape_elem == 4)
            TICK_TRY(vad::launch_tape_rows(rows_j, masked ? flags_j : nullptr, static_cast<float *>(p->d_tape), p->d_tape_clock, p->tape_chunks,
                                           p->streams, p->N, p->compute));
    }
    TICK_TRY(hipEventRecord(p->batch_free[buf], p->compute));
    TICK_TRY(hipEventRecord(p->tick_done[r], p->compute));
#undef TICK_TRY
    if (pk && pk->res)                           // what every listed stream carries after this tick; its first row binds it to its rate
        for (const vad_pump::Res &w : p->r_new) {
            p->n_bound += p->r_rate[w.stream] < 0;
            p->r_rate[w.stream] = w.rate;
            p->r_g[w.stream] = w.g, p->r_m[w.stream] = w.m, p->r_pend[w.stream] = w.pend;
        }
    else if (pk && pk->wide)                     // the pending counts and comb phases after this tick
        for (const vad_pump::Comb &w : p->w_new) {
            p->n_held += (w.now > 0) - (p->held[w.stream] > 0);
            p->held[w.stream] = w.now;
            p->w_step[w.stream] = w.step, p->w_phase[w.stream] = w.phase;
        }
    else if (pk && pk->burst)                    // the pending counts after this tick
        for (const vad_pump::Held &h : p->b_new) {
            p->n_held += (h.now > 0) - (p->held[h.stream] > 0);
            p->held[h.stream] = h.now;
        }
    else if (pk)                                 // (the table holds each row's count before it)
        for (long i = 0; i < n_rows; ++i) {
            const int32_t b = pk->stream[i], c = p->held[b] + pk->len[i];
            const int32_t now = c >= p->N ? c - p->N : c;
            p->n_held += (now > 0) - (p->held[b] > 0);
            p->held[b] = now;
        }
    p->batch_used[buf] = true;
    p->slot_busy[r] = 1;
    p->slot_steps[r] = steps;
    p->inflight.push_back(vad_pump::Flight{r, masked, steps});
    ++p->ticks;
    p->flips += steps;
    return VAD_OK;
}

}  // namespace

extern "C" {

int vad_pump_submit_present(vad_pump *p, int r, const uint8_t *present) { return submit_tick(p, r, present, false); }

int vad_pump_submit_compact(vad_pump *p, int r, const uint8_t *present) { return submit_tick(p, r, present, true); }

int vad_pump_submit_rows(vad_pump *p, int r, const int32_t *stream_of_row, long n_rows) {
    if (!p) return VAD_ERR_ARG;
    if (!stream_of_row && n_rows != 0) return pfail(p, VAD_ERR_ARG, "vad_pump_submit_rows: bad row list");
    static const int32_t none = 0;
    return submit_tick(p, r, nullptr, true, stream_of_row ? stream_of_row : &none, n_rows);
}

int vad_pump_submit(vad_pump *p, int r) { return submit_tick(p, r, nullptr, false); }

int vad_pump_submit_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *off_of_row, const int32_t *len_of_row,
                            long n_rows) {
    const Packets pk{stream_of_row, off_of_row, len_of_row};
    return submit_tick(p, r, nullptr, true, nullptr, n_rows, &pk);
}

int vad_pump_submit_coded_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row,
                                  const int32_t *len_of_row, const uint8_t *codec_of_row, long n_rows) {
    const Packets pk{stream_of_row, byte_off_of_row, len_of_row, true, codec_of_row};
    return submit_tick(p, r, nullptr, true, nullptr, n_rows, &pk);
}

int vad_pump_submit_burst(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row, const int32_t *len_of_row,
                          const uint8_t *codec_of_row, long n_rows) {
    Packets pk{stream_of_row, byte_off_of_row, len_of_row, true, codec_of_row};
    pk.burst = true;
    return submit_tick(p, r, nullptr, true, nullptr, n_rows, &pk);
}

int vad_pump_set_adpcm(vad_pump *p, int on) {
    if (!p) return VAD_ERR_ARG;
    if (on != 0 && on != 1) return pfail(p, VAD_ERR_ARG, "vad_pump_set_adpcm: on is 0 or 1");
    if (!p->inflight.empty()) return pfail(p, VAD_ERR_ARG, "vad_pump_set_adpcm: ticks in flight (retire them with vad_pump_poll first)");
    p->adpcm = on != 0;
    return VAD_OK;
}

int vad_pump_set_burst(vad_pump *p, int max_chunks) {
    if (!p) return VAD_ERR_ARG;
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (max_chunks < 1 || max_chunks > VAD_PUMP_MAX_BURST) return pfail(p, VAD_ERR_ARG, "vad_pump_set_burst: max_chunks out of 1 ... VAD_PUMP_MAX_BURST");
    if (!p->inflight.empty()) return pfail(p, VAD_ERR_ARG, "vad_pump_set_burst: ticks in flight (retire them with vad_pump_poll first)");
    if (max_chunks == p->max_burst) return VAD_OK;
    PUMP_TRY(p, hipSetDevice(p->device));
    PUMP_TRY(p, hipStreamSynchronize(p->compute));
    if (p->d_more) (void)hipFree(p->d_more);
    if (p->d_more_flags) (void)hipFree(p->d_more_flags);
    if (p->h_prob_more) (void)hipHostFree(p->h_prob_more);
    p->d_more = nullptr, p->d_more_flags = nullptr, p->h_prob_more = p->d_prob_more = nullptr;
    p->max_burst = 0;
    const size_t S = (size_t)p->streams, more = (size_t)max_chunks - 1;
    if (more > 0) {
        // (a sub-step computes every row, also the rows of the streams that are absent from it.  Rows no burst has filled yet must hold
        // samples, and NOT digital silence: behind a live stream's context a chunk of exact zeros is a chunk in which silence begins, and
        // the frontend evaluates those in double precision, ~0.1 ms a row (kernel_exact.hip).  A small constant is an ordinary chunk.)
        void *dv = nullptr;
        const bool ok = hipMalloc((void **)&p->d_more, more * S * p->N * sizeof(int16_t)) == hipSuccess &&
                        hipMalloc((void **)&p->d_more_flags, more * p->hdr) == hipSuccess &&
                        hipHostMalloc((void **)&p->h_prob_more, (size_t)p->R * more * S * sizeof(float), hipHostMallocMapped) == hipSuccess &&
                        hipMemsetD16(reinterpret_cast<hipDeviceptr_t>(p->d_more), 256, more * S * p->N) == hipSuccess &&
                        hipMemset(p->d_more_flags, 0, more * p->hdr) == hipSuccess &&
                        hipHostGetDevicePointer(&dv, p->h_prob_more, 0) == hipSuccess && dv && hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            if (p->d_more) (void)hipFree(p->d_more);
            if (p->d_more_flags) (void)hipFree(p->d_more_flags);
            if (p->h_prob_more) (void)hipHostFree(p->h_prob_more);
            p->d_more = nullptr, p->d_more_flags = nullptr, p->h_prob_more = nullptr;
            return pfail(p, VAD_ERR_ALLOC, "vad_pump_set_burst: no memory for the sub-steps' buffers");
        }
        p->d_prob_more = static_cast<float *>(dv);
        std::fill(p->h_prob_more, p->h_prob_more + (size_t)p->R * more * S, VAD_PROB_ABSENT);
    }
    p->b_len.assign(S, 0);
    p->b_cnt.assign(S, 0);
    p->b_pos.assign(S, 0);
    p->b_touched.reserve(S);
    p->b_new.reserve(S);
    p->max_burst = max_chunks;
    return VAD_OK;
}

int vad_pump_burst_steps(const vad_pump *p, int r) { return (p && r >= 0 && r < p->R) ? p->slot_steps[r] : -1; }

const float *vad_pump_burst_probs(const vad_pump *p, int r, int j) {
    if (!p || r < 0 || r >= p->R || j < 0 || j >= std::max(1, p->max_burst)) return nullptr;
    return p->step_probs(r, j);
}

int vad_pump_submit_wide_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row, const int32_t *len_of_row,
                                 const uint8_t *step_of_row, long n_rows) {
    Packets pk{stream_of_row, byte_off_of_row, len_of_row, true};
    pk.wide = true;
    pk.step = step_of_row;
    return submit_tick(p, r, nullptr, true, nullptr, n_rows, &pk);
}

int vad_pump_set_wideband(vad_pump *p, int max_step) {
    if (!p) return VAD_ERR_ARG;
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (max_step < 2 || max_step > vad::kMaxWideStep) return pfail(p, VAD_ERR_ARG, "vad_pump_set_wideband: max_step is 2 (32 kHz) or 3 (48 kHz)");
    if (p->sr != 16000)                          // (the reference decimates multiples of 16000 only: utils_vad.py:39-42)
        return pfail(p, VAD_ERR_SAMPLE_RATE, "vad_pump_set_wideband: only a 16 kHz pump takes 32 / 48 kHz rows");
    if (!p->inflight.empty()) return pfail(p, VAD_ERR_ARG, "vad_pump_set_wideband: ticks in flight (retire them with vad_pump_poll first)");
    if (max_step == p->max_step) return VAD_OK;
    PUMP_TRY(p, hipSetDevice(p->device));
    PUMP_TRY(p, hipStreamSynchronize(p->compute));
    if (p->d_wide) (void)hipFree(p->d_wide);
    if (p->h_wide) (void)hipHostFree(p->h_wide);
    p->d_wide = p->h_wide = nullptr;
    p->max_step = 0;
    const size_t S = (size_t)p->streams;
    p->wtab = (S * 4 * sizeof(int32_t) + 4095) / 4096 * 4096;
    p->wide_bytes = p->wtab + p->hdr + S * p->N * max_step * sizeof(int16_t);
    if (hipHostMalloc((void **)&p->h_wide, (size_t)p->R * p->wide_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&p->d_wide, vad_pump::NB * p->wide_bytes) != hipSuccess) {
        if (p->h_wide) (void)hipHostFree(p->h_wide);
        p->d_wide = p->h_wide = nullptr;
        return pfail(p, VAD_ERR_ALLOC, "vad_pump_set_wideband: no memory for the wide slots");
    }
    std::memset(p->h_wide, 0, (size_t)p->R * p->wide_bytes);
    p->w_step.assign(S, 0);
    p->w_phase.assign(S, 0);
    p->w_new.reserve(S);
    p->max_step = max_step;
    return VAD_OK;
}

uint8_t *vad_pump_wide_slot(vad_pump *p, int r) {
    return (p && p->max_step && r >= 0 && r < p->R) ? p->wide_present(r) + p->hdr : nullptr;
}

int vad_pump_wide_phase(const vad_pump *p, int stream) {
    if (!p || !p->max_step || stream < 0 || stream >= p->streams) return -VAD_ERR_ARG;
    return p->w_phase[stream];
}

int vad_pump_submit_resampled_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row,
                                      const int32_t *len_of_row, const uint8_t *rate_of_row, long n_rows) {
    Packets pk{stream_of_row, byte_off_of_row, len_of_row, true};
    pk.res = true;
    pk.rate = rate_of_row;
    return submit_tick(p, r, nullptr, true, nullptr, n_rows, &pk);
}

int vad_pump_set_resample(vad_pump *p, const int *src_rates, int n_rates) {
    if (!p) return VAD_ERR_ARG;
    const std::string fn = "vad_pump_set_resample: ";
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (!src_rates || n_rates < 1 || n_rates > VAD_PUMP_MAX_RATES) return pfail(p, VAD_ERR_ARG, fn + "1 ... VAD_PUMP_MAX_RATES source rates");
    if (p->tape_elem == 2)                       // (a resampled tick steps an fp32 batch: an int16 tape of it would not be what the net saw)
        return pfail(p, VAD_ERR_ARG, fn + "the pump has a tape (vad_pump_set_tape), and the tape does not hold the resampled route's fp32 chunks");
    if (!p->inflight.empty()) return pfail(p, VAD_ERR_ARG, fn + "ticks in flight (retire them with vad_pump_poll first)");
    std::shared_ptr<const vad::ResampleHostTable> tabs[vad::kMaxPumpRates];
    long A = 0, hmax = 0;
    for (int k = 0; k < n_rates; ++k) {
        tabs[k] = vad::resample_table(src_rates[k], p->sr);
        if (!tabs[k] || tabs[k]->end.empty())
            return pfail(p, VAD_ERR_SAMPLE_RATE, fn + std::to_string(src_rates[k]) + " -> " + std::to_string(p->sr) + " Hz is not served (vad_resample_geometry)");
        for (int q = 0; q < k; ++q)
            if (src_rates[q] == src_rates[k]) return pfail(p, VAD_ERR_ARG, fn + "a rate listed twice");
        A = std::max(A, ((long)p->N * tabs[k]->g.O + tabs[k]->g.N - 1) / tabs[k]->g.N);      // the input samples of one chunk
        hmax = std::max(hmax, (long)tabs[k]->H);
    }
    A = (A + 7) / 8 * 8;
    const long hld = (hmax + 7) / 8 * 8;
    if ((size_t)(hld + A + 2 * p->N) * sizeof(float) > 65536)
        return pfail(p, VAD_ERR_SAMPLE_RATE, fn + "a chunk of the largest rate and its history do not fit the assembly kernel's 64 KiB of LDS");
    if (p->n_rates == n_rates && std::equal(src_rates, src_rates + n_rates, p->rates)) return VAD_OK;
    PUMP_TRY(p, hipSetDevice(p->device));
    PUMP_TRY(p, hipStreamSynchronize(p->compute));
    vad::PumpRates dev{};
    for (int k = 0; k < n_rates; ++k) {          // the engine's shared tables (vad_resample_reserve): made once per pair and engine image
        vad::ResampleDeviceTable t{};
        if (const int rc = vad::engine_resample_table(p->eng, src_rates[k], p->sr, &t)) return pfail(p, rc, fn + vad_last_error(p->eng));
        dev.taps[k] = t.taps, dev.first[k] = t.first;
        dev.O[k] = t.g.O, dev.N[k] = t.g.N, dev.K[k] = t.g.K, dev.H[k] = tabs[k]->H;
    }
    auto drop = [&] {
        if (p->d_res) (void)hipFree(p->d_res);
        if (p->h_res) (void)hipHostFree(p->h_res);
        if (p->d_fbatch) (void)hipFree(p->d_fbatch);
        if (p->d_fcarry) (void)hipFree(p->d_fcarry);
        if (p->d_hist) (void)hipFree(p->d_hist);
        p->d_res = p->h_res = nullptr, p->d_fbatch = p->d_fcarry = nullptr, p->d_hist = nullptr;
        p->n_rates = 0, p->n_bound = 0;
    };
    drop();                                      // (another set of rates: everything is made anew and every stream is unbound)
    const size_t S = (size_t)p->streams, N = (size_t)p->N;
    p->rtab = (S * vad::kResampleRowWords * sizeof(int32_t) + 4095) / 4096 * 4096;
    p->res_bytes = p->rtab + p->hdr + S * (size_t)A * sizeof(int16_t);
    // (a step computes every row, also the rows of streams that no resampled tick has filled yet: they hold a small constant, not digital
    // silence -- see vad_pump_set_burst)
    std::vector<float> quiet(S * N, 256.0f / 32768.0f);
    const bool ok = hipHostMalloc((void **)&p->h_res, (size_t)p->R * p->res_bytes, hipHostMallocDefault) == hipSuccess &&
                    hipMalloc((void **)&p->d_res, vad_pump::NB * p->res_bytes) == hipSuccess &&
                    hipMalloc((void **)&p->d_fbatch, S * N * sizeof(float)) == hipSuccess &&
                    hipMalloc((void **)&p->d_fcarry, S * N * sizeof(float)) == hipSuccess &&
                    hipMalloc((void **)&p->d_hist, S * (size_t)hld * sizeof(int16_t)) == hipSuccess &&
                    hipMemcpy(p->d_fbatch, quiet.data(), S * N * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemset(p->d_fcarry, 0, S * N * sizeof(float)) == hipSuccess &&
                    hipMemset(p->d_hist, 0, S * (size_t)hld * sizeof(int16_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        drop();
        (void)hipGetLastError();
        return pfail(p, VAD_ERR_ALLOC, fn + "no memory for the resample slots");
    }
    std::memset(p->h_res, 0, (size_t)p->R * p->res_bytes);
    for (int k = 0; k < n_rates; ++k) p->rates[k] = src_rates[k], p->r_tab[k] = tabs[k];
    p->r_dev = dev;
    p->r_A = (int)A, p->r_hld = (int)hld;
    p->r_rate.assign(S, -1);
    p->r_g.assign(S, 0);
    p->r_m.assign(S, 0);
    p->r_pend.assign(S, 0);
    p->r_new.reserve(S);
    p->n_rates = n_rates;
    return VAD_OK;
}

uint8_t *vad_pump_resample_slot(vad_pump *p, int r) {
    return (p && p->n_rates && r >= 0 && r < p->R) ? p->res_present(r) + p->hdr : nullptr;
}

int vad_pump_resample_state(const vad_pump *p, int stream, int *src_rate, long *inputs_mod, long *pending) {
    if (!p || !p->n_rates || stream < 0 || stream >= p->streams) return VAD_ERR_ARG;
    const int k = p->r_rate[stream];
    if (src_rate) *src_rate = k < 0 ? 0 : p->rates[k];
    if (inputs_mod) *inputs_mod = k < 0 ? 0 : p->r_g[stream];
    if (pending) *pending = k < 0 ? 0 : p->r_pend[stream];
    return VAD_OK;
}

long vad_decimate(int step, int phase, const int16_t *in, long n, int16_t *out) {
    if (step < 1 || phase < 0 || phase >= step || n < 0 || (n > 0 && (!in || !out))) return -VAD_ERR_ARG;
    long m = 0;
    for (long k = vad::comb_first(step, phase); k < n; k += step) out[m++] = in[k];
    return m;
}

int vad_g711_expand(int codec, const uint8_t *in, long n, int16_t *out) {
    if (codec < VAD_PCM_S16 || codec > VAD_PCM_ALAW || n < 0 || (n > 0 && (!in || !out))) return VAD_ERR_ARG;
    if (codec == VAD_PCM_S16) {
        if (n > 0) std::memmove(out, in, (size_t)n * sizeof(int16_t));
        return VAD_OK;
    }
    for (long i = 0; i < n; ++i) out[i] = vad::g711_to_s16(codec, in[i]);
    return VAD_OK;
}

long vad_adpcm_expand(const uint8_t *payload, long nbytes, int16_t *out) {
    const long n = vad::adpcm_expand_serial(payload, nbytes, out);
    return n < 0 ? -VAD_ERR_ARG : n;
}

long vad_deinterleave(int codec, int channels, int channel, const void *in, long frames, int16_t *out) {
    if (codec < VAD_PCM_S16 || codec > VAD_PCM_ALAW || channels < 1 || channels > VAD_MAX_CHANNELS || channel < 0 || channel >= channels ||
        frames < 0 || (frames > 0 && (!in || !out)))
        return -VAD_ERR_ARG;
    if (codec == VAD_PCM_S16) {
        const uint8_t *b = static_cast<const uint8_t *>(in) + 2 * channel;       // (any even address: read bytewise)
        for (long i = 0; i < frames; ++i) std::memcpy(out + i, b + (size_t)i * 2 * channels, 2);
    } else {
        const uint8_t *b = static_cast<const uint8_t *>(in) + channel;
        for (long i = 0; i < frames; ++i) out[i] = vad::g711_to_s16(codec, b[(size_t)i * channels]);
    }
    return frames;
}

long vad_pump_pending(const vad_pump *p, int stream) {
    if (!p || stream < 0 || stream >= p->streams) return -1;
    return p->bound(stream) ? p->r_pend[stream] : p->held[stream];      // (a bound stream's pending samples are its fp32 outputs)
}

long vad_pump_poll(vad_pump *p, int block, vad_iter_event *out, long cap, int *slot) {
    if (!p || cap < 0 || (cap > 0 && !out)) return VAD_PUMP_ERROR;
    if (p->inflight.empty()) return VAD_PUMP_IDLE;
    const vad_pump::Flight f = p->inflight.front();
    const int r = f.r;
    if (block) {
        if (hipEventSynchronize(p->tick_done[r]) != hipSuccess) {
            pfail(p, VAD_ERR_HIP, "hipEventSynchronize(tick_done)");
            return VAD_PUMP_ERROR;
        }
    } else {
        const hipError_t q = hipEventQuery(p->tick_done[r]);
        if (q == hipErrorNotReady) return VAD_PUMP_BUSY;
        if (q != hipSuccess) {
            pfail(p, VAD_ERR_HIP, "hipEventQuery(tick_done)");
            return VAD_PUMP_ERROR;
        }
    }
    p->inflight.pop_front();
    p->slot_busy[r] = 0;
    if (slot) *slot = r;
    apply_ops(p);                                // opens / closes issued before this tick was submitted take effect with it
    long m = 0;
    for (int j = 0; j < f.steps; ++j) {          // (one step; a burst tick: one iterator call per sub-step, its events behind the earlier ones)
        const uint8_t *mask = p->active.data();
        if (f.masked) {                          // a stream without a chunk this step: no model call, no iterator call (utils_vad.py:507-549)
            const uint8_t *pr = p->slot_present(r);                              // (0 / 1; a burst tick: the chunks the stream completed)
            for (int s = 0; s < p->streams; ++s) p->feed_mask[s] = p->active[s] & (pr[s] > j);
            mask = p->feed_mask.data();
        }
        const long at = std::min(m, cap);
        m += vad_iterator_feed(p->step_probs(r, j), mask, p->streams, p->N, p->threshold, p->min_silence, p->pad, p->triggered.data(),
                               p->temp_end.data(), p->current.data(), out ? out + at : nullptr, cap - at);
    }
    ++p->retired;
    if (p->inflight.empty()) {                   // nothing in flight: later opens / closes have nothing to wait for
        p->retired = p->ticks;
        apply_ops(p);
    }
    return m;
}

int vad_pump_open(vad_pump *p, int stream) {
    if (!p) return VAD_ERR_ARG;
    if (stream < 0 || stream >= p->streams) return pfail(p, VAD_ERR_ARG, "vad_pump_open: no such stream");
    PUMP_TRY(p, hipSetDevice(p->device));
    // zero (h, c) and the context the NEXT tick reads, ordered behind the ticks already submitted (the compute stream)
    int k = 0;
    while (stream >= p->hi[k]) ++k;
    const size_t n = (size_t)(p->hi[k] - p->lo[k]), row = (size_t)(stream - p->lo[k]);
    PUMP_TRY(p, hipMemsetAsync(p->d_state[k] + row * 128, 0, 128 * sizeof(float), p->compute));
    PUMP_TRY(p, hipMemsetAsync(p->d_state[k] + (n + row) * 128, 0, 128 * sizeof(float), p->compute));
    PUMP_TRY(p, hipMemsetAsync(p->d_ctx[p->flips & 1] + (size_t)stream * p->C, 0, (size_t)p->C * sizeof(float), p->compute));
    if (p->tape_chunks)                          // ... and the tape's clock: the new stream's chunk 0 is the next one stepped here
        PUMP_TRY(p, hipMemsetAsync(p->d_tape_clock + 2 * (size_t)stream, 0, 2 * sizeof(int64_t), p->compute));
    p->drop_held(stream);                       // (the device carry needs nothing: the next packet tick's table says 0 samples pending)
    if (p->max_step) p->w_step[stream] = p->w_phase[stream] = 0;                // ... and the new stream's comb starts at its first sample
    if (p->n_rates) {                            // ... it is bound to no rate, and its filter history is zeros: "inputs before 0 are zero"
        PUMP_TRY(p, hipMemsetAsync(p->d_hist + (size_t)stream * p->r_hld, 0, (size_t)p->r_hld * sizeof(int16_t), p->compute));
        p->unbind(stream);
    }
    // ... and the host side (iterator state, active flag) when those ticks have been retired: their probabilities belong to the slot's
    // previous occupant and must neither advance the new stream's sample counter nor open a segment for it
    p->pending.push_back(vad_pump::Op{p->ticks, stream, true});
    if (p->inflight.empty()) {
        p->retired = p->ticks;
        apply_ops(p);
    }
    return VAD_OK;
}

int vad_pump_close(vad_pump *p, int stream) {
    if (!p) return VAD_ERR_ARG;
    if (stream < 0 || stream >= p->streams) return pfail(p, VAD_ERR_ARG, "vad_pump_close: no such stream");
    // the slot is still computed (lock-step batch) but emits no events -- from the next tick submitted on: the ticks in flight carry
    // chunks the stream did deliver, their events are still its own; samples it has pending are dropped
    p->drop_held(stream);
    if (p->bound(stream)) {                      // (a resampled stream: unbound, its pending outputs dropped, its history zero for the slot's next user)
        PUMP_TRY(p, hipSetDevice(p->device));
        PUMP_TRY(p, hipMemsetAsync(p->d_hist + (size_t)stream * p->r_hld, 0, (size_t)p->r_hld * sizeof(int16_t), p->compute));
        p->unbind(stream);
    }
    p->pending.push_back(vad_pump::Op{p->ticks, stream, false});
    if (p->inflight.empty()) {
        p->retired = p->ticks;
        apply_ops(p);
    }
    return VAD_OK;
}

int vad_pump_state(vad_pump *p, int stream, float *h, float *c, float *ctx) {
    if (!p) return VAD_ERR_ARG;
    if (stream < 0 || stream >= p->streams) return pfail(p, VAD_ERR_ARG, "vad_pump_state: no such stream");
    PUMP_TRY(p, hipSetDevice(p->device));
    PUMP_TRY(p, hipStreamSynchronize(p->compute));
    int k = 0;
    while (stream >= p->hi[k]) ++k;
    const size_t n = (size_t)(p->hi[k] - p->lo[k]), row = (size_t)(stream - p->lo[k]);
    if (h) PUMP_TRY(p, hipMemcpy(h, p->d_state[k] + row * 128, 128 * sizeof(float), hipMemcpyDeviceToHost));
    if (c) PUMP_TRY(p, hipMemcpy(c, p->d_state[k] + (n + row) * 128, 128 * sizeof(float), hipMemcpyDeviceToHost));
    if (ctx) PUMP_TRY(p, hipMemcpy(ctx, p->d_ctx[p->flips & 1] + (size_t)stream * p->C, (size_t)p->C * sizeof(float), hipMemcpyDeviceToHost));
    return VAD_OK;
}

}  // extern "C"

// The tape (include/silero_vad_hip.h "THE TAPE"; kernel_tape.hip; the window rule: tape.hpp)
namespace {

// every counter as of all the ticks submitted so far: the compute stream is drained first
int tape_read_clock(vad_pump *p) {
    PUMP_TRY(p, hipSetDevice(p->device));
    PUMP_TRY(p, hipStreamSynchronize(p->compute));
    PUMP_TRY(p, hipMemcpy(p->tape_clock.data(), p->d_tape_clock, (size_t)p->streams * 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return VAD_OK;
}

// room for n requests, and (host destination) for `bytes` of packed samples
int tape_reserve(vad_pump *p, size_t n, size_t bytes) {
    if (n > p->tape_req_cap) {
        if (p->d_tape_req) (void)hipFree(p->d_tape_req);
        if (p->h_tape_req) (void)hipHostFree(p->h_tape_req);
        p->d_tape_req = p->h_tape_req = nullptr, p->tape_req_cap = 0;
        const size_t cap = std::max<size_t>(n, 256);
        if (hipHostMalloc((void **)&p->h_tape_req, cap * sizeof(vad::TapeRequest), hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void **)&p->d_tape_req, cap * sizeof(vad::TapeRequest)) != hipSuccess) {
            if (p->h_tape_req) (void)hipHostFree(p->h_tape_req);
            p->d_tape_req = p->h_tape_req = nullptr;
            (void)hipGetLastError();
            return pfail(p, VAD_ERR_ALLOC, "vad_pump_fetch_audio: no memory for the request table");
        }
        p->tape_req_cap = cap;
    }
    if (bytes > p->tape_out_cap) {
        if (p->d_tape_out) (void)hipFree(p->d_tape_out);
        if (p->h_tape_out) (void)hipHostFree(p->h_tape_out);
        p->d_tape_out = p->h_tape_out = nullptr, p->tape_out_cap = 0;
        if (hipMalloc((void **)&p->d_tape_out, bytes) != hipSuccess ||
            hipHostMalloc((void **)&p->h_tape_out, bytes, hipHostMallocDefault) != hipSuccess) {
            if (p->d_tape_out) (void)hipFree(p->d_tape_out);
            p->d_tape_out = p->h_tape_out = nullptr;
            (void)hipGetLastError();
            return pfail(p, VAD_ERR_ALLOC, "vad_pump_fetch_audio: no memory to stage the samples");
        }
        p->tape_out_cap = bytes;
    }
    return VAD_OK;
}

// vad_pump_set_tape (elem = 2) and vad_pump_set_tape_f32 (elem = 4): one tape a pump, of either element
int tape_set(vad_pump *p, int chunks, int elem, const std::string &fn) {
    if (!p) return VAD_ERR_ARG;
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (chunks < 2) return pfail(p, VAD_ERR_ARG, fn + "a tape holds at least 2 chunks a stream");
    if (p->tape_chunks) return pfail(p, VAD_ERR_ARG, fn + "the pump has its tape already");
    if (p->ticks > 0) return pfail(p, VAD_ERR_ARG, fn + "only before the pump's first tick: the tape's clock is the count of every chunk stepped");
    if (elem == 2 && p->n_rates)                 // (a resampled tick steps an fp32 batch: an int16 tape of it would not be what the net saw)
        return pfail(p, VAD_ERR_ARG, fn + "the pump takes resampled rows (vad_pump_set_resample), and the tape does not hold that route's fp32 chunks");
    PUMP_TRY(p, hipSetDevice(p->device));
    const size_t S = (size_t)p->streams;
    void *tape = nullptr;
    int64_t *clock = nullptr;
    const bool ok = hipMalloc(&tape, S * (size_t)chunks * p->N * (size_t)elem) == hipSuccess &&
                    hipMalloc((void **)&clock, S * 2 * sizeof(int64_t)) == hipSuccess &&
                    hipMemset(clock, 0, S * 2 * sizeof(int64_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        if (tape) (void)hipFree(tape);
        if (clock) (void)hipFree(clock);
        (void)hipGetLastError();
        return pfail(p, VAD_ERR_ALLOC, fn + "no device memory for streams x chunks x N samples");
    }
    p->d_tape = tape, p->d_tape_clock = clock;
    p->tape_clock.assign(S * 2, 0);
    p->tape_chunks = chunks, p->tape_elem = elem;
    return VAD_OK;
}

// vad_pump_fetch_audio (T = int16_t) and vad_pump_fetch_audio_f32 (T = float); offsets and counts are in elements of T
template <typename T>
int tape_fetch(vad_pump *p, const int32_t *stream, const int64_t *first, const int64_t *count, long n, const int64_t *out_offset, T *out,
               int out_on_device, const std::string &fn) {
    if (!p) return VAD_ERR_ARG;
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (!p->tape_chunks) return pfail(p, VAD_ERR_ARG, fn + "the pump has no tape (vad_pump_set_tape)");
    if (p->tape_elem != (int)sizeof(T))
        return pfail(p, VAD_ERR_ARG, fn + (p->tape_elem == 4 ? "the pump's tape is float32 (vad_pump_set_tape_f32): fetch it with vad_pump_fetch_audio_f32"
                                                             : "the pump's tape is int16 (vad_pump_set_tape): fetch it with vad_pump_fetch_audio"));
    if (n < 0 || (n > 0 && (!stream || !first || !count || !out_offset))) return pfail(p, VAD_ERR_ARG, fn + "bad request list");
    int64_t max_count = 0, total = 0;
    for (long i = 0; i < n; ++i) {
        if (stream[i] < 0 || stream[i] >= p->streams) return pfail(p, VAD_ERR_ARG, fn + "request " + std::to_string(i) + ": no such stream");
        if (count[i] < 0 || out_offset[i] < 0) return pfail(p, VAD_ERR_ARG, fn + "request " + std::to_string(i) + ": a negative count or offset");
        max_count = std::max(max_count, count[i]);
    }
    if (max_count == 0) return VAD_OK;           // (nothing to copy: no request has a sample)
    if (!out) return pfail(p, VAD_ERR_ARG, fn + "no destination");
    if (const int rc = tape_read_clock(p)) return rc;
    // the same rule, against the counters as they are NOW: a tick submitted since vad_pump_tape_window may have taped over the range
    constexpr int64_t V = 16 / (int64_t)sizeof(T);     // elements of 16 bytes: every staged request starts on a multiple of it
    for (long i = 0; i < n; ++i) {
        if (count[i] == 0) continue;
        const int64_t *c = p->tape_clock.data() + 2 * (size_t)stream[i];
        const int64_t lo = vad::tape_held_lo(c[0], c[1], p->tape_chunks, p->N), hi = vad::tape_held_hi(c[0], p->N);
        if (first[i] < lo || first[i] > hi || count[i] > hi - first[i])
            return pfail(p, VAD_ERR_ARG, fn + "request " + std::to_string(i) + ": samples " + std::to_string(first[i]) + " ... of stream " +
                                             std::to_string(stream[i]) + " are no longer held (the tape holds " + std::to_string(lo) + " ... " +
                                             std::to_string(hi) + ")");
        total += (count[i] + V - 1) / V * V;
    }
    if (const int rc = tape_reserve(p, (size_t)n, out_on_device ? 0 : (size_t)total * sizeof(T))) return rc;
    int64_t at = 0;
    for (long i = 0; i < n; ++i) {               // host destination: packed on the device, every request 16-byte aligned
        p->h_tape_req[i] = vad::TapeRequest{stream[i], first[i], count[i], out_on_device ? out_offset[i] : at};
        at += (count[i] + V - 1) / V * V;
    }
    // read-only behind everything the compute stream has run: a failure leaves the pump as it was
    T *d_out = out_on_device ? out : reinterpret_cast<T *>(p->d_tape_out);
    const T *h_out = reinterpret_cast<const T *>(p->h_tape_out);
    PUMP_TRY(p, hipMemcpyAsync(p->d_tape_req, p->h_tape_req, (size_t)n * sizeof(vad::TapeRequest), hipMemcpyHostToDevice, p->compute));
    PUMP_TRY(p, vad::launch_tape_gather(p->d_tape_req, n, (long)max_count, static_cast<const T *>(p->d_tape), p->tape_chunks, p->N, d_out, p->compute));
    if (!out_on_device) PUMP_TRY(p, hipMemcpyAsync(p->h_tape_out, p->d_tape_out, (size_t)total * sizeof(T), hipMemcpyDeviceToHost, p->compute));
    PUMP_TRY(p, hipStreamSynchronize(p->compute));
    for (long i = 0; i < n && !out_on_device; ++i)       // exactly count[i] samples each: what lies between the requests is not touched
        if (count[i] > 0) std::memcpy(out + out_offset[i], h_out + p->h_tape_req[i].out_offset, (size_t)count[i] * sizeof(T));
    return VAD_OK;
}

}  // namespace

extern "C" {

int vad_tape_window(int64_t count, int64_t floor, int chunks, int N, int64_t start, int64_t end, int64_t *first, int64_t *n) {
    // (count * N and floor * N must be int64 values: everything else about the rule is clamps)
    if (chunks < 2 || N < 1 || count < 0 || count > INT64_MAX / N || floor < INT64_MIN / N || floor > INT64_MAX / N || start > end || !first || !n)
        return VAD_ERR_ARG;
    vad::tape_window(count, floor, chunks, N, start, end, first, n);
    return VAD_OK;
}

int vad_tape_run(int64_t count, int64_t floor, int chunks, int N, int64_t from, int64_t *first_chunk, int64_t *n_chunks) {
    if (chunks < 2 || N < 1 || count < 0 || count > INT64_MAX / N || floor < 0 || floor > INT64_MAX / N || !first_chunk || !n_chunks) return VAD_ERR_ARG;
    vad::tape_run(count, floor, chunks, N, from, first_chunk, n_chunks);
    return VAD_OK;
}

int vad_pump_set_tape(vad_pump *p, int chunks) { return tape_set(p, chunks, (int)sizeof(int16_t), "vad_pump_set_tape: "); }

int vad_pump_set_tape_f32(vad_pump *p, int chunks) { return tape_set(p, chunks, (int)sizeof(float), "vad_pump_set_tape_f32: "); }

int vad_pump_tape_format(const vad_pump *p) { return p ? p->tape_elem : -VAD_ERR_ARG; }

int vad_pump_tape_state(vad_pump *p, int stream, int64_t *count, int64_t *floor) {
    if (!p) return VAD_ERR_ARG;
    if (!p->tape_chunks) return pfail(p, VAD_ERR_ARG, "vad_pump_tape_state: the pump has no tape (vad_pump_set_tape)");
    if (stream < 0 || stream >= p->streams) return pfail(p, VAD_ERR_ARG, "vad_pump_tape_state: no such stream");
    if (const int rc = tape_read_clock(p)) return rc;
    if (count) *count = p->tape_clock[2 * (size_t)stream];
    if (floor) *floor = p->tape_clock[2 * (size_t)stream + 1];
    return VAD_OK;
}

long vad_pump_tape_window(vad_pump *p, const int32_t *stream, const int64_t *start, const int64_t *end, long n, int64_t *first, int64_t *count) {
    if (!p) return -VAD_ERR_ARG;
    const std::string fn = "vad_pump_tape_window: ";
    if (!p->tape_chunks) return -pfail(p, VAD_ERR_ARG, fn + "the pump has no tape (vad_pump_set_tape)");
    if (n < 0 || (n > 0 && (!stream || !start || !end || !first || !count))) return -pfail(p, VAD_ERR_ARG, fn + "bad request list");
    for (long i = 0; i < n; ++i) {               // (before anything is written, and before the pump is made to wait)
        if (stream[i] < 0 || stream[i] >= p->streams) return -pfail(p, VAD_ERR_ARG, fn + "request " + std::to_string(i) + ": no such stream");
        if (start[i] > end[i]) return -pfail(p, VAD_ERR_ARG, fn + "request " + std::to_string(i) + ": start behind end");
    }
    if (const int rc = tape_read_clock(p)) return -rc;
    long total = 0;
    for (long i = 0; i < n; ++i) {
        const int64_t *c = p->tape_clock.data() + 2 * (size_t)stream[i];
        vad::tape_window(c[0], c[1], p->tape_chunks, p->N, start[i], end[i], first + i, count + i);
        total += (long)count[i];
    }
    return total;
}

int vad_pump_fetch_audio(vad_pump *p, const int32_t *stream, const int64_t *first, const int64_t *count, long n, const int64_t *out_offset,
                         int16_t *out, int out_on_device) {
    return tape_fetch(p, stream, first, count, n, out_offset, out, out_on_device, "vad_pump_fetch_audio: ");
}

int vad_pump_fetch_audio_f32(vad_pump *p, const int32_t *stream, const int64_t *first, const int64_t *count, long n, const int64_t *out_offset,
                             float *out, int out_on_device) {
    return tape_fetch(p, stream, first, count, n, out_offset, out, out_on_device, "vad_pump_fetch_audio_f32: ");
}

}  // extern "C"

// Snapshot and restore (include/silero_vad_hip.h "SNAPSHOT AND RESTORE"; kernel_snapshot.hip).  The blob's header and record layout:
namespace {

#if __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "the snapshot blob is little-endian and is written from the host's own representation"
#endif
struct SnapHeader {
    char magic[8];
    uint32_t version, header_bytes;
    int32_t sr, N, C;
    uint32_t stride;
    int64_t n_records;
    double threshold, min_silence, pad;
};
static_assert(sizeof(SnapHeader) == VAD_SNAPSHOT_HEADER_BYTES && sizeof(vad_stream_info) == 32, "the blob layout is the documented one");
static_assert(sizeof(vad_resample_info) == 32 && VAD_SNAPSHOT_HEADER_BYTES_V2 % 16 == 0 && vad::kSnapHistory == VAD_SNAPSHOT_HISTORY &&
                  vad::kResampleMaxTaps <= VAD_SNAPSHOT_HISTORY,
              "the version 2 tail is the documented one, and holds the history of every served pair");
const char kSnapMagic[8] = {'S', 'V', 'A', 'D', 'S', 'N', 'A', 'P'};

// Where everything of a blob of `version` lies -- the one place that knows what a version adds.  A record is vad_stream_info, h, c, the
// context and the pending samples; from version 2 on, behind them, the tail: vad_resample_info, float carry[N], int16
// history[VAD_SNAPSHOT_HISTORY]; in version 3, behind that, vad_tape_info, and the header goes on with {int32 tape_elem, int32 reserved,
// int64 tape_bytes} and zeros, the tape section follows the records.
struct SnapLayout {
    size_t header_bytes, stride;
    size_t tail_at, run_at;                      // of vad_resample_info and of vad_tape_info in a record; 0: this version has none
    int table_words;                             // of a record's entry in the kernels' work table (device_api.hpp)
};
constexpr SnapLayout snap_layout(int version, int N, int C) {
    const size_t v1 = sizeof(vad_stream_info) + (size_t)(2 * 128 + C) * sizeof(float) + (size_t)N * sizeof(int16_t);
    const size_t v2 = v1 + sizeof(vad_resample_info) + (size_t)N * sizeof(float) + VAD_SNAPSHOT_HISTORY * sizeof(int16_t);
    return version == VAD_SNAPSHOT_VERSION_3   ? SnapLayout{VAD_SNAPSHOT_HEADER_BYTES_V3, v2 + sizeof(vad_tape_info), v1, v2, 8}
           : version == VAD_SNAPSHOT_VERSION_2 ? SnapLayout{VAD_SNAPSHOT_HEADER_BYTES_V2, v2, v1, 0, 8}
                                               : SnapLayout{VAD_SNAPSHOT_HEADER_BYTES, v1, 0, 0, 4};
}
static_assert(snap_layout(1, 512, 64).header_bytes == sizeof(SnapHeader) && snap_layout(1, 512, 64).stride == 2336 && snap_layout(1, 256, 32).stride == 1696,
              "the version 1 layout is the documented one");
static_assert(snap_layout(2, 512, 64).stride == 4736 && snap_layout(2, 512, 64).tail_at == snap_layout(1, 512, 64).stride && snap_layout(2, 256, 32).stride % 16 == 0,
              "the version 2 layout is the documented one: the version 1 record goes first");
static_assert(sizeof(vad_tape_info) == 32 && sizeof(vad::SnapRun) == 32 && snap_layout(3, 512, 64).header_bytes == sizeof(SnapHeader) + 64 &&
                  snap_layout(3, 512, 64).run_at == snap_layout(2, 512, 64).stride && snap_layout(3, 512, 64).stride == snap_layout(2, 512, 64).stride + 32,
              "the version 3 layout is the documented one: the version 2 record goes first");
struct SnapTape {                                // what a version 3 header says of the tape section (versions 1 and 2: no tape)
    int32_t elem = 0;
    int64_t bytes = 0;
};
// A blob that snap_check has accepted (it may lie at any address: everything is read through memcpy).
struct SnapBlob {
    SnapHeader hd;
    SnapLayout at;
    SnapTape tape;
    const uint8_t *rec = nullptr;                // record 0; the tape section lies behind record n_records - 1
    const uint8_t *record(long r) const { return rec + (size_t)r * at.stride; }
    const uint8_t *tape_section() const { return record((long)hd.n_records); }
    template <class T>
    T part(long r, size_t where, bool has) const {               // (a version without the part: zeros -- bound to no rate, no run)
        T x{};
        if (has) std::memcpy(&x, record(r) + where, sizeof(x));
        return x;
    }
    vad_stream_info info(long r) const { return part<vad_stream_info>(r, 0, true); }
    vad_resample_info tail(long r) const { return part<vad_resample_info>(r, at.tail_at, at.tail_at != 0); }
    vad_tape_info run(long r) const { return part<vad_tape_info>(r, at.run_at, at.run_at != 0); }
};

bool any_byte_set(const uint8_t *at, size_t n) {
    uint8_t acc = 0;
    for (size_t i = 0; i < n; ++i) acc |= at[i];
    return acc != 0;
}

// The tail of a record whose info block is `f` (all of it, like everything of a blob, is read through memcpy).  *last: the pair looked
// up last, so that a blob of 8 192 records of a few rates takes the table's lock a few times.
struct SnapPair {
    int rate = 0;
    std::shared_ptr<const vad::ResampleHostTable> tab;
};
const char *snap_tail_fault(const uint8_t *tail, const vad_stream_info &f, int sr, int N, SnapPair *last) {
    vad_resample_info q;
    std::memcpy(&q, tail, sizeof(q));
    for (const uint8_t z : q.reserved)
        if (z) return "reserved bytes that are not zero";
    long c = 0, H = 0;                           // the live floats of the carry, the pair's history
    if (q.src_rate == 0) {
        if (q.pending_out || q.inputs_mod || q.outputs_mod) return "resample counters of a stream that is bound to no rate";
    } else {
        if (q.src_rate != last->rate) last->rate = q.src_rate, last->tab = q.src_rate > 0 ? vad::resample_table(q.src_rate, sr) : nullptr;
        if (!last->tab || last->tab->end.empty()) return "a src_rate that is not served for the blob's sample rate";
        const vad::ResampleHostTable &t = *last->tab;
        if (q.pending_out < 0 || q.pending_out >= N) return "pending_out out of 0 ... N - 1";
        if (q.outputs_mod < 0 || q.outputs_mod >= t.g.N) return "outputs_mod out of 0 ... the pair's N - 1";
        if (q.inputs_mod < 0 || q.inputs_mod >= t.end.back()) return "inputs_mod below 0, or so large that a whole period would be ready";
        if (vad::resample_stream_ready(t, q.inputs_mod) != q.outputs_mod) return "outputs_mod is not what a stream of inputs_mod inputs has emitted";
        if (f.pending != 0) return "a stream that is bound to a rate with int16 samples pending";
        c = q.pending_out, H = t.H;
    }
    const uint8_t *carry = tail + sizeof(q), *hist = carry + (size_t)N * sizeof(float);
    if (any_byte_set(carry + (size_t)c * sizeof(float), (size_t)(N - c) * sizeof(float))) return "a float behind pending_out that is not +0.0f";
    if (any_byte_set(hist + (size_t)H * sizeof(int16_t), (size_t)(VAD_SNAPSHOT_HISTORY - H) * sizeof(int16_t))) return "a history sample behind H that is not zero";
    return nullptr;
}

const char *snap_info_fault(const vad_stream_info &f, int N) {
    if (f.pending < 0 || f.pending >= N) return "pending out of 0 ... N - 1";
    if (f.active > 1 || f.triggered > 1) return "active / triggered other than 0 / 1";
    if (f.wide_step > vad::kMaxWideStep) return "wide_step above 3";
    if (f.wide_phase >= std::max<int>(1, f.wide_step)) return "wide_phase not below max(1, wide_step)";
    if (f.current_sample < 0 || f.temp_end < 0 || f.temp_end > f.current_sample) return "current_sample / temp_end out of range";
    for (const uint8_t z : f.reserved)
        if (z) return "reserved bytes that are not zero";
    return nullptr;
}

// The vad_tape_info of a record whose info block is `f`.  *done: the chunks of the earlier runs; total: the chunks the tape
// section holds, tape_bytes / (N * elem) (0 without a tape).  Every comparison comes before the arithmetic it makes safe.
const char *snap_run_fault(const uint8_t *at, const vad_stream_info &f, int N, int elem, int64_t total, int64_t *done) {
    vad_tape_info t;
    std::memcpy(&t, at, sizeof(t));
    for (const uint8_t z : t.reserved)
        if (z) return "reserved bytes that are not zero";
    if (t.first_chunk < 0 || t.n_chunks < 0) return "a run with a negative first_chunk or n_chunks";
    if (t.n_chunks == 0) {
        if (t.first_chunk != 0 || t.offset != 0) return "an empty run whose first_chunk or offset is not zero";
    } else {
        if (elem == 0) return "a run in a blob without a tape";
        if (t.n_chunks > total - *done) return "runs longer than the tape section";
        if (t.offset != *done * N * elem) return "a run that does not start where the run before it ends";       // (*done <= total: the product is below tape_bytes)
        if (f.current_sample % N != 0 || t.first_chunk != f.current_sample / N - t.n_chunks) return "a run that does not end at the record's current_sample";
        *done += t.n_chunks;
    }
    return nullptr;
}

// The whole blob, header and every record's fields.  -> nullptr and *b, the view of it, or what is wrong with it.
const char *snap_check(const void *blob, size_t nbytes, SnapBlob *b) {
    SnapHeader &hd = b->hd;
    if (!blob || nbytes < sizeof(SnapHeader)) return "shorter than a header";
    std::memcpy(&hd, blob, sizeof(SnapHeader));
    if (std::memcmp(hd.magic, kSnapMagic, sizeof(kSnapMagic)) != 0) return "not a snapshot (magic)";
    if (hd.version < VAD_SNAPSHOT_VERSION || hd.version > VAD_SNAPSHOT_VERSION_3 || hd.header_bytes != snap_layout((int)hd.version, 0, 0).header_bytes)
        return "a version this library does not read";
    if (nbytes < hd.header_bytes) return "shorter than a header";
    const uint8_t *bytes = static_cast<const uint8_t *>(blob);
    const bool runs = snap_layout((int)hd.version, 0, 0).run_at != 0;
    SnapTape &tape = b->tape = SnapTape{};
    size_t zeros = sizeof(SnapHeader);           // the header is zeros from here on
    if (runs) {                                  // {int32 tape_elem, int32 reserved, int64 tape_bytes}
        int32_t word[2];
        std::memcpy(word, bytes + zeros, sizeof(word));
        std::memcpy(&tape.bytes, bytes + zeros + sizeof(word), sizeof(tape.bytes));
        tape.elem = word[0], zeros += 16;
        if (word[1] != 0) return "reserved bytes that are not zero";
    }
    if (any_byte_set(bytes + zeros, hd.header_bytes - zeros)) return "reserved bytes that are not zero";
    if (tape.elem != 0 && tape.elem != 2 && tape.elem != 4) return "a tape_elem other than 0, 2 or 4";
    if (tape.bytes < 0 || (tape.elem == 0 && tape.bytes != 0)) return "tape_bytes below zero, or not zero without a tape";
    int N = 0, C = 0;
    if (vad_geometry(hd.sr, &N, &C) != VAD_OK || hd.N != N || hd.C != C || hd.stride != snap_layout((int)hd.version, N, C).stride)
        return "a sample rate / geometry that does not exist";
    b->at = snap_layout((int)hd.version, N, C);
    b->rec = bytes + hd.header_bytes;
    if (hd.n_records < 0 || (uint64_t)hd.n_records > (nbytes - hd.header_bytes) / hd.stride) return "shorter than its header claims";
    // with a tape section the buffer is exactly the header, the records and that section
    if (runs && (uint64_t)tape.bytes != nbytes - hd.header_bytes - (size_t)hd.n_records * hd.stride) return "not as long as its header claims";
    const int64_t total = tape.elem ? tape.bytes / ((int64_t)N * tape.elem) : 0;
    int64_t done = 0;
    SnapPair last;
    for (int64_t i = 0; i < hd.n_records; ++i) {
        const vad_stream_info f = b->info((long)i);
        if (const char *why = snap_info_fault(f, N)) return why;
        if (b->at.tail_at)
            if (const char *why = snap_tail_fault(b->record((long)i) + b->at.tail_at, f, hd.sr, N, &last)) return why;
        if (b->at.run_at)
            if (const char *why = snap_run_fault(b->record((long)i) + b->at.run_at, f, N, tape.elem, total, &done)) return why;
    }
    if (tape.elem && done * N * tape.elem != tape.bytes) return "a tape section that is not the sum of its runs";
    return nullptr;
}

int part_of(const vad_pump *p, int b) { return (int)(std::upper_bound(p->hi.begin(), p->hi.end(), b) - p->hi.begin()); }

// One staging of a call: its table (first call: `entries` of T, page-locked and mapped, the kernels read it in place) and room for
// `bytes` on the device.
template <class T>
int snap_stage(vad_pump *p, T **h_tab, T **d_tab, size_t entries, uint8_t **d_buf, size_t *cap, size_t bytes, const char *no_table, const char *no_room) {
    PUMP_TRY(p, hipSetDevice(p->device));
    if (!*h_tab) {
        void *dv = nullptr;
        T *tab = nullptr;
        if (hipHostMalloc((void **)&tab, entries * sizeof(T), hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dv, tab, 0) != hipSuccess || !dv) {
            if (tab) (void)hipHostFree(tab);
            (void)hipGetLastError();
            return pfail(p, VAD_ERR_ALLOC, no_table);
        }
        *h_tab = tab, *d_tab = static_cast<T *>(dv);
    }
    if (bytes > *cap) {
        if (*d_buf) (void)hipFree(*d_buf);
        *d_buf = nullptr, *cap = 0;
        if (hipMalloc((void **)d_buf, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return pfail(p, VAD_ERR_ALLOC, no_room);
        }
        *cap = bytes;
    }
    return VAD_OK;
}

// the records: the work table (8 words a stream: room for an entry with a tail), the packed records and the part table (first call)
int snap_reserve(vad_pump *p, size_t bytes) {
    if (const int rc = snap_stage(p, &p->h_snap_tab, &p->d_snap_tab, (size_t)p->streams * 8, &p->d_snap, &p->snap_cap, bytes,
                                  "snapshot: no memory for the work tables", "snapshot: no device memory for the records"))
        return rc;
    if (!p->d_snap_parts) {
        std::vector<vad::SnapPart> parts;
        for (int k = 0; k < p->parts; ++k) parts.push_back(vad::SnapPart{p->d_state[k], p->lo[k], p->hi[k] - p->lo[k]});
        vad::SnapPart *dp = nullptr;
        if (hipMalloc((void **)&dp, parts.size() * sizeof(vad::SnapPart)) != hipSuccess ||
            hipMemcpy(dp, parts.data(), parts.size() * sizeof(vad::SnapPart), hipMemcpyHostToDevice) != hipSuccess) {
            if (dp) (void)hipFree(dp);
            (void)hipGetLastError();
            return pfail(p, VAD_ERR_ALLOC, "snapshot: no memory for the work tables");
        }
        p->d_snap_parts = dp;
    }
    return VAD_OK;
}

// the runs of the tape: the table of runs and the packed chunks
int snap_tape_reserve(vad_pump *p, size_t bytes) {
    return snap_stage(p, &p->h_snap_runs, &p->d_snap_runs, (size_t)p->streams, &p->d_snap_tape, &p->snap_tape_cap, bytes,
                      "snapshot: no memory for the table of runs", "snapshot: no device memory to stage the runs of the tape");
}

// A record's entry of the work table: {slot, part, pending, record} and, in a layout with a tail, {c, H, bound, 0} behind it.
void snap_entry(vad_pump *p, const SnapLayout &at, long k, int32_t slot, int32_t pending, int32_t record, int32_t c, int32_t H, bool bound) {
    int32_t *e = p->h_snap_tab + at.table_words * k;
    e[0] = slot, e[1] = part_of(p, slot), e[2] = pending, e[3] = record;
    if (at.table_words == 8) e[4] = c, e[5] = H, e[6] = bound, e[7] = 0;
}

// the tail arguments of the record kernels (null: records without a tail)
const vad::SnapTail *snap_tail_args(const vad_pump *p, const SnapLayout &at, vad::SnapTail *tl) {
    if (!at.tail_at) return nullptr;
    *tl = vad::SnapTail{p->d_fcarry, p->d_hist, p->r_hld, at.run_at ? (int)(at.stride - at.run_at) : 0};    // (what lies behind the tail is the host's)
    return tl;
}

// both calls: not on a poisoned pump, not with a tick in flight
int snap_idle(vad_pump *p, const std::string &fn) {
    if (p->poisoned) return pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")");
    if (!p->inflight.empty()) return pfail(p, VAD_ERR_ARG, fn + "ticks in flight (retire them with vad_pump_poll first)");
    return VAD_OK;
}

// the slot list of an export: 0 = fine, 1 = a bad count, 2 = a slot out of range or listed twice
int snap_slots_fault(vad_pump *p, const int32_t *streams, long n) {
    const long S = p->streams;
    if (n < 0 || n > S || (!streams && n != S && n != 0)) return 1;
    bool bad = false;
    long i = 0;
    for (; streams && i < n && !bad; ++i) {
        const int32_t b = streams[i];
        if (!(bad = b < 0 || b >= S || p->seen[b])) p->seen[b] = 1;
    }
    for (long k = 0; streams && k < i; ++k)      // (only valid slots were marked)
        if (streams[k] >= 0 && streams[k] < S) p->seen[streams[k]] = 0;
    return bad ? 2 : 0;
}

// The runs a version 3 export of these (checked) slots carries, as the counters are NOW (synchronises) -> run[k] = {first_chunk, n_chunks,
// offset in chunks} and their chunks together.  A stream whose tape clock is not its iterator clock, and every stream of a pump
// without a tape, carries none.
struct SnapRunPlan {
    int64_t first, n, at;
};
int snap_plan_runs(vad_pump *p, const int32_t *streams, long n, const int64_t *tape_from, std::vector<SnapRunPlan> *run, int64_t *total) {
    run->assign((size_t)n, SnapRunPlan{0, 0, 0});
    *total = 0;
    if (!p->tape_chunks || n == 0) return VAD_OK;
    if (const int rc = tape_read_clock(p)) return rc;
    for (long k = 0; k < n; ++k) {
        const int32_t b = streams ? streams[k] : (int32_t)k;
        const int64_t count = p->tape_clock[2 * (size_t)b], floor = p->tape_clock[2 * (size_t)b + 1];
        if (count < 0 || floor < 0 || count > INT64_MAX / p->N || count * p->N != p->current[b]) continue;
        SnapRunPlan &q = (*run)[(size_t)k];
        vad::tape_run(count, floor, p->tape_chunks, p->N, tape_from ? tape_from[k] : INT64_MIN, &q.first, &q.n);
        if (q.n == 0) q.first = 0;               // (an empty run is all zeros in the blob)
        else q.at = *total, *total += q.n;
    }
    return VAD_OK;
}

// vad_pump_export_streams, vad_pump_export_streams_v2 and vad_pump_export_streams_v3 (version = 1, 2, 3)
const char *const kExportName[] = {"vad_pump_export_streams: ", "vad_pump_export_streams_v2: ", "vad_pump_export_streams_v3: "};
const char *const kExportNeeds[] = {"vad_pump_snapshot_bytes(sr, n)", "vad_pump_snapshot_bytes_v2(sr, n)", "vad_pump_snapshot_plan_v3(p, streams, n, tape_from)"};

int snap_export(vad_pump *p, const int32_t *streams, long n, void *blob, size_t cap, int version, const int64_t *tape_from = nullptr) {
    if (!p) return VAD_ERR_ARG;
    const std::string fn = kExportName[version - 1];
    if (const int rc = snap_idle(p, fn)) return rc;
    const int slots = snap_slots_fault(p, streams, n);
    if (slots == 1 || !blob) return pfail(p, VAD_ERR_ARG, fn + "bad slot list (NULL = every slot: n is then the pump's stream count) or no blob");
    if (slots) return pfail(p, VAD_ERR_ARG, fn + "a slot out of range, or listed twice");
    const SnapLayout at = snap_layout(version, p->N, p->C);
    const size_t stride = at.stride;
    std::vector<SnapRunPlan> run;
    int64_t run_chunks = 0;
    if (at.run_at)
        if (const int rc = snap_plan_runs(p, streams, n, tape_from, &run, &run_chunks)) return rc;
    const size_t row_bytes = (size_t)p->N * (size_t)p->tape_elem, tape_bytes = (size_t)run_chunks * row_bytes;       // (run_chunks <= streams x chunks: the tape itself is that large)
    if (cap < at.header_bytes + (size_t)n * stride + tape_bytes) return pfail(p, VAD_ERR_ARG, fn + "the blob needs " + kExportNeeds[version - 1] + " bytes");
    for (long k = 0; !at.tail_at && k < n && p->n_bound > 0; ++k)
        if (p->r_rate[streams ? streams[k] : k] >= 0)
            return pfail(p, VAD_ERR_ARG, fn + "stream " + std::to_string(streams ? streams[k] : k) + " is bound to a resampled rate: blob version 1 has no room for "
                                                  "its fp32 pending outputs and filter history (vad_pump_export_streams_v2 writes version 2)");
    uint8_t *rec = static_cast<uint8_t *>(blob) + at.header_bytes;
    if (n > 0) {
        if (const int rc = snap_reserve(p, (size_t)n * stride)) return rc;
        if (run_chunks > 0)
            if (const int rc = snap_tape_reserve(p, tape_bytes)) return rc;
        for (long k = 0; k < n; ++k) {
            const int32_t b = streams ? streams[k] : (int32_t)k;
            const bool is_bound = p->bound(b);
            snap_entry(p, at, k, b, p->held[b], (int32_t)k, is_bound ? p->r_pend[b] : 0, is_bound ? p->r_tab[p->r_rate[b]]->H : 0, is_bound);
        }
        // (read-only, behind everything the compute stream has run: a failure leaves the pump as it was)
        vad::SnapTail tl;
        PUMP_TRY(p, vad::launch_snapshot_gather(p->d_snap_tab, n, p->d_snap_parts, p->d_ctx[p->flips & 1], p->d_carry, p->N, p->C, p->d_snap, p->compute,
                                                snap_tail_args(p, at, &tl)));
        PUMP_TRY(p, hipMemcpyAsync(rec, p->d_snap, (size_t)n * stride, hipMemcpyDeviceToHost, p->compute));
        if (run_chunks > 0) {                    // the runs: packed on the device in record order, ONE copy into the tape section
            int64_t longest = 0;
            for (long k = 0; k < n; ++k) {       // (n <= chunks by the run rule; [at, at + n) inside the staging by the sum)
                const SnapRunPlan &q = run[(size_t)k];
                p->h_snap_runs[k] = vad::SnapRun{streams ? streams[k] : (int32_t)k, (int32_t)q.n, q.first, q.at, 0};
                longest = std::max(longest, q.n);
            }
            PUMP_TRY(p, vad::launch_snapshot_tape(false, p->d_snap_runs, n, (long)longest, p->d_tape, p->tape_chunks, p->N, p->tape_elem, p->d_snap_tape, p->compute));
            PUMP_TRY(p, hipMemcpyAsync(rec + (size_t)n * stride, p->d_snap_tape, tape_bytes, hipMemcpyDeviceToHost, p->compute));
        }
        PUMP_TRY(p, hipStreamSynchronize(p->compute));
    }
    SnapHeader hd;
    std::memcpy(hd.magic, kSnapMagic, sizeof(kSnapMagic));
    hd.version = (uint32_t)version, hd.header_bytes = (uint32_t)at.header_bytes;
    hd.sr = p->sr, hd.N = p->N, hd.C = p->C, hd.stride = (uint32_t)stride, hd.n_records = n;
    hd.threshold = p->threshold, hd.min_silence = p->min_silence, hd.pad = p->pad;
    std::memcpy(blob, &hd, sizeof(hd));
    std::memset(static_cast<uint8_t *>(blob) + sizeof(hd), 0, at.header_bytes - sizeof(hd));
    if (at.run_at) {
        const int32_t elem = p->tape_elem;
        const int64_t tb = (int64_t)tape_bytes;
        std::memcpy(static_cast<uint8_t *>(blob) + sizeof(hd), &elem, sizeof(elem));
        std::memcpy(static_cast<uint8_t *>(blob) + sizeof(hd) + 8, &tb, sizeof(tb));
    }
    for (long k = 0; k < n; ++k) {               // the host's parts of a record (the gather left them zero)
        const int32_t b = streams ? streams[k] : (int32_t)k;
        vad_stream_info f{};
        f.current_sample = p->current[b], f.temp_end = p->temp_end[b], f.pending = p->held[b];
        f.active = p->active[b], f.triggered = p->triggered[b];
        if (p->max_step) f.wide_step = p->w_step[b], f.wide_phase = p->w_phase[b];
        std::memcpy(rec + (size_t)k * stride, &f, sizeof(f));
        if (at.tail_at && p->bound(b)) {
            vad_resample_info q{};
            q.src_rate = p->rates[p->r_rate[b]], q.pending_out = p->r_pend[b], q.inputs_mod = p->r_g[b], q.outputs_mod = p->r_m[b];
            std::memcpy(rec + (size_t)k * stride + at.tail_at, &q, sizeof(q));
        }
        if (at.run_at && run[(size_t)k].n > 0) {
            vad_tape_info t{};
            t.first_chunk = run[(size_t)k].first, t.n_chunks = run[(size_t)k].n, t.offset = run[(size_t)k].at * (int64_t)row_bytes;
            std::memcpy(rec + (size_t)k * stride + at.run_at, &t, sizeof(t));
        }
    }
    return VAD_OK;
}

// header + n records of `version`; 0 for arguments no blob has
size_t snap_bytes(int version, int sr, long n) {
    int N = 0, C = 0;
    if (n < 0 || vad_geometry(sr, &N, &C) != VAD_OK) return 0;
    const SnapLayout at = snap_layout(version, N, C);
    return at.header_bytes + (size_t)n * at.stride;
}

}  // namespace

extern "C" {

size_t vad_pump_snapshot_bytes(int sr, long n) { return snap_bytes(1, sr, n); }

size_t vad_pump_snapshot_bytes_v2(int sr, long n) { return snap_bytes(2, sr, n); }

size_t vad_snapshot_bytes_v3(int sr, long n, int tape_elem, int64_t total_chunks) {
    int N = 0, C = 0;
    if (n < 0 || vad_geometry(sr, &N, &C) != VAD_OK || (tape_elem != 0 && tape_elem != 2 && tape_elem != 4) || total_chunks < 0 ||
        (tape_elem == 0 && total_chunks != 0))
        return 0;
    const SnapLayout at = snap_layout(3, N, C);
    const size_t row = (size_t)N * (size_t)tape_elem;
    if ((size_t)n > (SIZE_MAX - at.header_bytes) / at.stride) return 0;
    const size_t records = at.header_bytes + (size_t)n * at.stride;
    if (row && (uint64_t)total_chunks > (SIZE_MAX - records) / row) return 0;
    return records + (size_t)total_chunks * row;
}

int vad_snapshot_inspect(const void *blob, size_t nbytes, long *n_records, int *sr) {
    SnapBlob b;
    if (snap_check(blob, nbytes, &b)) return VAD_ERR_ARG;
    if (n_records) *n_records = (long)b.hd.n_records;
    if (sr) *sr = b.hd.sr;
    return VAD_OK;
}

int vad_snapshot_stream(const void *blob, size_t nbytes, long i, vad_stream_info *info, float *h, float *c, float *ctx, int16_t *pending) {
    SnapBlob b;
    if (snap_check(blob, nbytes, &b) || i < 0 || i >= b.hd.n_records) return VAD_ERR_ARG;
    const uint8_t *rec = b.record(i);
    const size_t st = 128 * sizeof(float), cx = (size_t)b.hd.C * sizeof(float);
    if (info) *info = b.info(i);
    if (h) std::memcpy(h, rec + sizeof(vad_stream_info), st);
    if (c) std::memcpy(c, rec + sizeof(vad_stream_info) + st, st);
    if (ctx) std::memcpy(ctx, rec + sizeof(vad_stream_info) + 2 * st, cx);
    if (pending) std::memcpy(pending, rec + sizeof(vad_stream_info) + 2 * st + cx, (size_t)b.hd.N * sizeof(int16_t));
    return VAD_OK;
}

int vad_snapshot_resample(const void *blob, size_t nbytes, long i, vad_resample_info *info, float *carry, int16_t *history) {
    SnapBlob b;
    if (snap_check(blob, nbytes, &b) || i < 0 || i >= b.hd.n_records) return VAD_ERR_ARG;
    const size_t cb = (size_t)b.hd.N * sizeof(float), hb = VAD_SNAPSHOT_HISTORY * sizeof(int16_t);
    if (info) *info = b.tail(i);
    if (!b.at.tail_at) {                         // (a record without a tail: the stream is bound to no rate)
        if (carry) std::memset(carry, 0, cb);
        if (history) std::memset(history, 0, hb);
        return VAD_OK;
    }
    const uint8_t *rows = b.record(i) + b.at.tail_at + sizeof(vad_resample_info);
    if (carry) std::memcpy(carry, rows, cb);
    if (history) std::memcpy(history, rows + cb, hb);
    return VAD_OK;
}

int vad_snapshot_tape(const void *blob, size_t nbytes, long i, vad_tape_info *info, void *audio, size_t cap) {
    SnapBlob b;
    if (snap_check(blob, nbytes, &b) || i < 0 || i >= b.hd.n_records) return VAD_ERR_ARG;
    const vad_tape_info t = b.run(i);
    const size_t bytes = (size_t)t.n_chunks * (size_t)b.hd.N * (size_t)b.tape.elem;     // (snap_check: inside the tape section)
    if (audio && cap < bytes) return VAD_ERR_ARG;
    if (info) *info = t;
    if (audio && bytes) std::memcpy(audio, b.tape_section() + (size_t)t.offset, bytes);
    return VAD_OK;
}

int vad_pump_export_streams(vad_pump *p, const int32_t *streams, long n, void *blob, size_t cap) { return snap_export(p, streams, n, blob, cap, 1); }

int vad_pump_export_streams_v2(vad_pump *p, const int32_t *streams, long n, void *blob, size_t cap) { return snap_export(p, streams, n, blob, cap, 2); }

size_t vad_pump_snapshot_plan_v3(vad_pump *p, const int32_t *streams, long n, const int64_t *tape_from) {
    if (!p) return 0;
    const std::string fn = "vad_pump_snapshot_plan_v3: ";
    if (p->poisoned) return (void)pfail(p, VAD_ERR_HIP, "the pump failed half-way through an earlier tick; destroy it (" + p->err + ")"), 0;
    if (snap_slots_fault(p, streams, n)) return (void)pfail(p, VAD_ERR_ARG, fn + "bad slot list (NULL = every slot: n is then the pump's stream count; distinct slots)"), 0;
    std::vector<SnapRunPlan> run;
    int64_t run_chunks = 0;
    if (snap_plan_runs(p, streams, n, tape_from, &run, &run_chunks)) return 0;
    const SnapLayout at = snap_layout(3, p->N, p->C);
    return at.header_bytes + (size_t)n * at.stride + (size_t)run_chunks * (size_t)p->N * (size_t)p->tape_elem;
}

int vad_pump_export_streams_v3(vad_pump *p, const int32_t *streams, long n, const int64_t *tape_from, void *blob, size_t cap) {
    return snap_export(p, streams, n, blob, cap, 3, tape_from);
}

int vad_pump_import_streams(vad_pump *p, const void *blob, size_t nbytes, const int32_t *records, const int32_t *streams, long n) {
    if (!p) return VAD_ERR_ARG;
    const std::string fn = "vad_pump_import_streams: ";
    if (const int rc = snap_idle(p, fn)) return rc;
    SnapBlob in;
    if (const char *why = snap_check(blob, nbytes, &in)) return pfail(p, VAD_ERR_ARG, fn + "the blob is " + why);
    const SnapHeader &hd = in.hd;
    const SnapTape &tape = in.tape;
    if (hd.sr != p->sr) return pfail(p, VAD_ERR_SAMPLE_RATE, fn + "the blob's sample rate is not the pump's");
    if (tape.elem && p->tape_elem && tape.elem != p->tape_elem)
        return pfail(p, VAD_ERR_ARG, fn + (tape.elem == 2 ? "the blob carries runs of an int16 tape and the pump's tape is float32"
                                                          : "the blob carries runs of a float32 tape and the pump's tape is int16") +
                                         ": an import does not convert");
    const long S = p->streams;
    if (n < 0 || n > S || (n > 0 && !streams)) return pfail(p, VAD_ERR_ARG, fn + "bad slot list");
    const size_t stride = hd.stride;
    // the runs of the blob's tape section enter this pump's tape, the newest tape_chunks chunks of each: without a tape here none is kept
    // (with one, its element is the blob's by now)
    const size_t row_bytes = (size_t)p->N * (size_t)p->tape_elem;
    auto rate_index = [&](int src_rate) {        // among THIS pump's rates; -1: not enabled here
        for (int k = 0; k < p->n_rates; ++k)
            if (p->rates[k] == src_rate) return k;
        return -1;
    };
    // everything is decided here, on the host, from values snap_check has range-checked: nothing is queued before the last check
    const char *why = nullptr;
    long i = 0, first = hd.n_records, last = -1;
    int64_t run_lo = INT64_MAX, run_hi = 0, longest = 0;       // the span of the selected runs in the tape section, in bytes; the longest kept run
    for (; i < n && !why; ++i) {
        const long r = records ? records[i] : i;
        const int32_t b = streams[i];
        if (r < 0 || r >= hd.n_records) why = "a record index out of range";
        else if (b < 0 || b >= S || p->seen[b]) why = "a slot out of range, or listed twice";
        else if (in.info(r).wide_step >= 2 && in.info(r).wide_step > p->max_step) why = "a record of a 32 / 48 kHz stream, and the pump's wideband max_step is smaller (vad_pump_set_wideband)";
        else if (in.tail(r).src_rate && rate_index(in.tail(r).src_rate) < 0) why = "a record of a stream that is bound to a rate this pump has not enabled (vad_pump_set_resample)";
        else {
            p->seen[b] = 1;
            first = std::min(first, r), last = std::max(last, r);
            const vad_tape_info t = in.run(r);
            if (t.n_chunks > 0) {
                run_lo = std::min(run_lo, t.offset), run_hi = std::max(run_hi, t.offset + t.n_chunks * (int64_t)row_bytes);
                longest = std::max(longest, std::min<int64_t>(t.n_chunks, p->tape_chunks));
            }
        }
    }
    for (long k = 0; k < i; ++k)                 // (only valid slots were marked)
        if (streams[k] >= 0 && streams[k] < S) p->seen[streams[k]] = 0;
    if (why) return pfail(p, VAD_ERR_ARG, fn + why);
    if (n == 0) return VAD_OK;
    const size_t bytes = (size_t)(last - first + 1) * stride;
    if (const int rc = snap_reserve(p, bytes)) return rc;
    if (longest > 0)
        if (const int rc = snap_tape_reserve(p, (size_t)(run_hi - run_lo))) return rc;
    for (long k = 0; k < n && longest > 0; ++k) {                  // the newest `kept` chunks of each run, into this pump's own ring
        const vad_tape_info t = in.run(records ? records[k] : k);
        const int64_t kept = std::min<int64_t>(t.n_chunks, p->tape_chunks), skip = t.n_chunks - kept;
        p->h_snap_runs[k] = vad::SnapRun{streams[k], (int32_t)kept, t.first_chunk + skip, kept ? (t.offset - run_lo) / (int64_t)row_bytes + skip : 0, 0};
    }
    for (long k = 0; k < n; ++k) {
        const long r = records ? records[k] : k;
        const vad_resample_info q = in.tail(r);    // (snap_check has held c and the pair against their ranges; H <= this pump's pitch: the rate is enabled here)
        snap_entry(p, in.at, k, streams[k], in.info(r).pending, (int32_t)(r - first), q.pending_out, q.src_rate ? p->r_tab[rate_index(q.src_rate)]->H : 0,
                   q.src_rate != 0);
    }
    // ONE copy: the records first ... last; the scatter behind it on the compute stream.  From the copy on a failure leaves slots
    // half-replaced: the pump says so from then on.
    const hipError_t rc = [&] {
        vad::SnapTail tl;
        hipError_t e = hipMemcpyAsync(p->d_snap, in.record(first), bytes, hipMemcpyHostToDevice, p->compute);
        if (e == hipSuccess)
            e = vad::launch_snapshot_scatter(p->d_snap_tab, n, p->d_snap_parts, p->d_ctx[p->flips & 1], p->d_carry, p->N, p->C, p->d_snap, p->compute,
                                             snap_tail_args(p, in.at, &tl));
        if (e == hipSuccess && longest > 0) {    // ONE more copy: the tape section from the first selected run to the last; the scatter behind it
            e = hipMemcpyAsync(p->d_snap_tape, in.tape_section() + (size_t)run_lo, (size_t)(run_hi - run_lo), hipMemcpyHostToDevice, p->compute);
            if (e == hipSuccess)
                e = vad::launch_snapshot_tape(true, p->d_snap_runs, n, (long)longest, p->d_tape, p->tape_chunks, p->N, p->tape_elem, p->d_snap_tape, p->compute);
        }
        return e == hipSuccess ? hipStreamSynchronize(p->compute) : e;
    }();
    if (rc != hipSuccess) {
        p->poisoned = true;
        return pfail(p, VAD_ERR_HIP, fn + hipGetErrorString(rc));
    }
    for (long k = 0; k < n; ++k) {               // the host's part of the slot
        const vad_stream_info f = in.info(records ? records[k] : k);
        const int32_t b = streams[k];
        p->active[b] = f.active, p->triggered[b] = f.triggered, p->temp_end[b] = f.temp_end, p->current[b] = f.current_sample;
        p->n_held += (f.pending > 0) - (p->held[b] > 0);
        p->held[b] = f.pending;
        if (p->max_step) p->w_step[b] = f.wide_step, p->w_phase[b] = f.wide_phase;
        const vad_resample_info q = in.tail(records ? records[k] : k);
        if (q.src_rate) {                        // a bound record: the scatter wrote the slot's whole carry and history rows
            p->n_bound += p->r_rate[b] < 0;
            p->r_rate[b] = (int8_t)rate_index(q.src_rate);
            p->r_g[b] = (long)q.inputs_mod, p->r_m[b] = (long)q.outputs_mod, p->r_pend[b] = q.pending_out;
        } else if (p->bound(b)) {                // (the slot's previous stream was a resampled one: the imported stream is bound to no rate)
            (void)hipMemsetAsync(p->d_hist + (size_t)b * p->r_hld, 0, (size_t)p->r_hld * sizeof(int16_t), p->compute);
            p->unbind(b);
        }
        p->src_pos[b] = 0;
    }
    if (p->tape_chunks) {                        // the stream's clock continues: count = its chunk; floor = count less the chunks of its run that were
                                                 // kept (a version 3 record with a run), else count: nothing before the import is held
        const size_t bytes2 = (size_t)S * 2 * sizeof(int64_t);                 // (the pump is idle and synchronised: nothing else writes the counters)
        hipError_t e = hipMemcpy(p->tape_clock.data(), p->d_tape_clock, bytes2, hipMemcpyDeviceToHost);
        for (long k = 0; k < n; ++k) {
            const int64_t count = p->current[streams[k]] / p->N;
            p->tape_clock[2 * (size_t)streams[k]] = count;
            p->tape_clock[2 * (size_t)streams[k] + 1] = count - std::min<int64_t>(in.run(records ? records[k] : k).n_chunks, p->tape_chunks);
        }
        if (e == hipSuccess) e = hipMemcpy(p->d_tape_clock, p->tape_clock.data(), bytes2, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            p->poisoned = true;
            return pfail(p, VAD_ERR_HIP, fn + hipGetErrorString(e));
        }
    }
    return VAD_OK;
}

// The whole loop, natively.  SOURCE threads play the part of the audio sources: thread k owns a range of streams and, for every tick,
// WRITES their chunks into the tick's ring slot (rows -> slot; streaming stores: the data is bound for the DMA engine, not for this
// core's cache) as soon as the server has room for the tick -- the memory traffic an audio server's receive path causes.  The
// calling thread is the server loop: wait until the slot is completely written, submit the tick, and once `depth` ticks are in
// flight retire the oldest (wait, iterator logic, events).  depth 1: strictly one tick at a time -- the next chunks are written
// after the previous tick's events are out, so "written -> events" is the latency of ONE tick.  depth >= 2: the sources write the
// tick that comes next while `depth` ticks are in flight (they run depth + 1 ticks ahead of the retired ones).
// Both sides BLOCK when they have to wait (Gate: 20 us of spinning, then a futex): the sources on the count of retired ticks, the
// server on the count of sources that have written the slot.
}  // extern "C"

namespace {

long play_loop(vad_pump *p, const int16_t *rows, long ld, long period, const uint8_t *pattern, long pattern_ticks, long first_tick,
               long n_ticks, int depth, int fill_threads, vad_iter_event *out, long cap, vad_pump_stats *st, bool compact) {
    if (!p) return VAD_PUMP_ERROR;
    const long N = p->N;
    if (!rows || ld < period || period < N || period % N || first_tick < 0 || n_ticks < 0 || cap < 0 || (cap > 0 && !out) ||
        (pattern && pattern_ticks <= 0)) {
        pfail(p, VAD_ERR_ARG, "vad_pump_play: bad argument");
        return VAD_PUMP_ERROR;
    }
    if (!p->inflight.empty()) {
        pfail(p, VAD_ERR_ARG, "vad_pump_play: ticks in flight (retire them with vad_pump_poll first)");
        return VAD_PUMP_ERROR;
    }
    depth = std::max(1, std::min(depth, p->R - 1));
    const long ahead = depth == 1 ? 1 : depth + 1;                             // <= R: the slot's previous tick has been retired by then
    const bool silent = fill_threads < 0;        // diagnostic: the sources write nothing (the slots keep their content): device side only
    int nsrc = fill_threads > 0 ? fill_threads : std::max(1, std::min(8, vad::default_host_threads(32) - 2));
    nsrc = std::max(1, std::min(nsrc, (p->streams + 63) / 64));
    const long per = ((p->streams + nsrc - 1) / nsrc + 15) / 16 * 16;          // whole tiles per source thread
    const long last = first_tick + n_ticks;
    std::atomic<long> retired{first_tick};
    std::vector<std::atomic<int>> written(p->R);
    for (auto &w : written) w.store(0);
    std::atomic<bool> stop{false};
    std::atomic<long> fill_ns{0}, chunks{0};
    Gate room, filled;                           // room: a tick was retired (sources wait); filled: a source finished a slot (server waits)
    auto source = [&](int k) {
        const long b0 = std::min<long>(p->streams, k * per), b1 = std::min<long>(p->streams, b0 + per);
        long mine = 0;
        for (long t = first_tick; t < last; ++t) {
            room.wait([&] { return t - retired.load(std::memory_order_acquire) < ahead || stop.load(std::memory_order_relaxed); });
            if (stop.load(std::memory_order_relaxed)) return;
            if (!silent && b1 > b0) {
                const double f0 = now_ms();
                const int r = (int)(t % p->R);
                int16_t *slot = p->slot_pcm(r);
                if (!pattern) {
                    const long off = (t * N) % period;
                    for (long b = b0; b < b1; ++b)
                        stream_copy(slot + b * N, rows + b * ld + off, (size_t)N * sizeof(int16_t), b + 1 < b1 ? rows + (b + 1) * ld + off : nullptr);
                    mine += b1 - b0;
                } else {
                    // stream b has a chunk this tick iff its flag says so; its audio advances only then (a late packet delays the
                    // stream's own next chunk, it does not skip audio)
                    const uint8_t *pat = pattern + (size_t)(t % pattern_ticks) * p->streams;
                    uint8_t *flags = p->slot_present(r);
                    // compact: the delivering streams' chunks lie back to back (vad_pump_submit_compact) -- this thread's first row
                    // is the number of streams before its range that deliver this tick
                    long row = 0;
                    if (compact)
                        for (long b = 0; b < b0; ++b) row += pat[b] != 0;
                    for (long b = b0; b < b1; ++b) {
                        flags[b] = pat[b];
                        if (!pat[b]) continue;
                        const long off = (p->src_pos[b]++ * N) % period;
                        stream_copy(slot + (compact ? row++ : b) * N, rows + b * ld + off, (size_t)N * sizeof(int16_t));
                        ++mine;
                    }
                }
                stream_fence();
                fill_ns.fetch_add((long)((now_ms() - f0) * 1e6), std::memory_order_relaxed);
            }
            written[t % p->R].fetch_add(1, std::memory_order_release);
            filled.signal();
        }
        chunks.fetch_add(mine, std::memory_order_relaxed);
    };
    std::vector<std::thread> sources;
    for (int k = 0; k < nsrc; ++k) sources.emplace_back(source, k);
    std::vector<double> t_written(p->R, 0.0), lat;
    lat.reserve((size_t)n_ticks);
    std::vector<vad_iter_event> scratch((size_t)p->streams);
    long n_events = 0;
    double wait_ms = 0.0, submit_ms = 0.0;
    bool ok = true;
    auto retire = [&]() -> bool {
        int r = -1;
        const double w0 = now_ms();
        const long m = vad_pump_poll(p, 1, scratch.data(), (long)scratch.size(), &r);
        const double w1 = now_ms();
        if (m < 0) return false;
        wait_ms += w1 - w0;
        lat.push_back(w1 - t_written[r]);
        for (long i = 0; i < m; ++i, ++n_events)
            if (n_events < cap) out[n_events] = scratch[i];
        retired.fetch_add(1, std::memory_order_release);
        room.signal();
        return true;
    };
    const double t0 = now_ms();
    for (long t = first_tick; t < last && ok; ++t) {
        const int r = (int)(t % p->R);
        filled.wait([&] { return written[r].load(std::memory_order_acquire) >= nsrc; });
        written[r].store(0, std::memory_order_relaxed);          // (the slot's next writers wait for this tick's retirement)
        const double s0 = now_ms();
        t_written[r] = s0;
        ok = submit_tick(p, r, pattern && !silent ? p->slot_present(r) : nullptr, compact && pattern && !silent) == VAD_OK;
        submit_ms += now_ms() - s0;
        if (ok && (int)p->inflight.size() >= depth) ok = retire();
    }
    while (ok && !p->inflight.empty()) ok = retire();
    const double t1 = now_ms();
    stop.store(true);
    room.signal();
    for (auto &th : sources) th.join();
    if (!ok) {
        (void)hipStreamSynchronize(p->compute);                                  // leave nothing in flight behind an error
        while (!p->inflight.empty()) {
            p->slot_busy[p->inflight.front().r] = 0;
            p->inflight.pop_front();
        }
        return VAD_PUMP_ERROR;
    }
    if (st) {
        std::sort(lat.begin(), lat.end());
        const size_t n = lat.size();
        st->ticks = n_ticks;
        st->events = n_events;
        st->wall_ms = t1 - t0;
        st->tick_ms_p50 = n ? lat[n / 2] : 0.0;
        st->tick_ms_p95 = n ? lat[std::min(n - 1, (size_t)(n * 0.95))] : 0.0;
        st->tick_ms_max = n ? lat[n - 1] : 0.0;
        st->fill_ms_mean = n_ticks ? (double)fill_ns.load() * 1e-6 / nsrc / n_ticks : 0.0;
        st->submit_ms_mean = n_ticks ? submit_ms / n_ticks : 0.0;
        st->wait_ms_mean = n_ticks ? wait_ms / n_ticks : 0.0;
        st->fill_threads = silent ? 0 : nsrc;
        st->depth = depth;
        st->chunks = silent ? (long)p->streams * n_ticks : chunks.load();
    }
    return n_events;
}

}  // namespace

extern "C" {

long vad_pump_play_gaps(vad_pump *p, const int16_t *rows, long ld, long period, const uint8_t *pattern, long pattern_ticks, long first_tick,
                        long n_ticks, int depth, int fill_threads, vad_iter_event *out, long cap, vad_pump_stats *st) {
    return play_loop(p, rows, ld, period, pattern, pattern_ticks, first_tick, n_ticks, depth, fill_threads, out, cap, st, false);
}

long vad_pump_play_compact(vad_pump *p, const int16_t *rows, long ld, long period, const uint8_t *pattern, long pattern_ticks, long first_tick,
                           long n_ticks, int depth, int fill_threads, vad_iter_event *out, long cap, vad_pump_stats *st) {
    return play_loop(p, rows, ld, period, pattern, pattern_ticks, first_tick, n_ticks, depth, fill_threads, out, cap, st, true);
}

long vad_pump_play(vad_pump *p, const int16_t *rows, long ld, long period, long first_tick, long n_ticks, int depth, int fill_threads,
                   vad_iter_event *out, long cap, vad_pump_stats *st) {
    return play_loop(p, rows, ld, period, nullptr, 0, first_tick, n_ticks, depth, fill_threads, out, cap, st, false);
}

}  // extern "C"
