// device_api.hpp -- launcher declarations shared by engine.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/silero_vad_hip.h"

namespace vad {

// device pointers to the canonical (un-packed) tensors of one net, for impl="reference"
struct RefNet {
    const float *basis;
    const float *ew[4], *eb[4];
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w_out, *b_out;
};

__device__ __forceinline__ float load_pcm(const float *p) { return *p; }
__device__ __forceinline__ float load_pcm(const int16_t *p) { return (float)(*p) * (1.0f / 32768.0f); }

template <typename PcmT>
hipError_t launch_ref_forward(const RefNet &w, int sr, int B, long L, const PcmT *pcm, long ld,
                              float *ctx, float *state, float *probs, long ldp, hipStream_t s);

// dst[b][i] = src[b][i * k] (the reference's x[:, ::step] for 32/48/... kHz input)
template <typename PcmT>
hipError_t launch_decimate(const PcmT *src, long lds, PcmT *dst, long ldd, int B, long Ld, int k, hipStream_t s);

// ---- product path --------------------------------------------------------------------------------
// Frontend: PCM -> in-wave FFT magnitude -> 4 conv blocks -> W_ih GEMM, fp32 MFMA.
//   one wave = 16 chunks (16 streams x one time step); gx is written in MFMA D-fragment order
//   gx[stream_tile][t][mblock 32][lane 64][4]   (stream_tile = 16 consecutive streams)
// Also writes ctx_out[b][C] = last C samples of the (zero padded) input of every stream.
struct FrontArgs {
    const float *wfront;     // packed GEMM stream (layout.hpp)
    const float *tables;     // biases, window, twiddles
    const void *pcm;         // [B][L] float or int16, rows 16-byte aligned
    const void *tail;        // [B][N] zero padded copy of the last chunk when L % N != 0, else null
    long ld, L, T;           // row stride (elements), samples per stream, chunks per stream
    long t0, nt;             // time slab [t0, t0 + nt) processed by this launch
    const float *ctx_in;     // [B][C] context of chunk 0 (read when t == 0)
    float *ctx_out;          // [B][C] written by the waves that own t == T-1 (may alias ctx_in)
    float *gx;               // scratch, tile-major, indexed with slab-relative t
    int B;
    int dec;                 // 0/1: pcm is at the net's rate; 2, 3: pcm is at 32 / 48 kHz and ld, pcm, tail index RAW samples --
                             // the kernel reads every dec-th one (fp32 frontends; 3: kernel_front_f43.hip only); L, T, t0, nt stay
                             // in 16 kHz terms
    long long *trace;        // bring-up only (VAD_TRACE builds): 16 slots per workgroup, else null
    // chunks that hold an exactly silent STFT frame beside one that is not (exact_front.hpp) get their gx from a double-precision
    // evaluation.  exact_net: the canonical fp32 tensors (device copy of RefNet), or null = the feature is off.  The latency frontend
    // computes such chunks itself; the throughput frontend appends their ids ((st * nt + tl) * 16 + j) to exact_list[1 + *exact_list],
    // and launch_exact_fix overwrites their columns of gx.  exact_list: [0] count, [1] workgroups done (both zero between launches),
    // [2 ...] ids.
    const RefNet *exact_net;
    int *exact_list;
    const float *gx_silent;  // [512] gx of a chunk of zeros with zero context (a constant of the net), or null: all-silent chunks keep the
                             // fp32 chains' value (option exact_transitions=edges; study mode)
};
// gx_silent of one net: exact_front.hpp's double-precision evaluation of a chunk of zeros, 512 floats to `out` (device).
hipError_t launch_exact_silent(int sr, const RefNet *net_dev, float *out, hipStream_t s);
// Behind a throughput-frontend launch with a.exact_list set: recompute the listed chunks (exact_front.hpp) into a.gx; resets the list.
template <typename PcmT>
hipError_t launch_exact_fix(int sr, const FrontArgs &a, hipStream_t s);
// (A/B form, test builds only -- VAD_AB, libsilero_vad_hip_ab.so: encoder 0 tap by tap, straight-line code, kernel_front.hip)
template <typename PcmT>
hipError_t launch_front(int sr, const FrontArgs &a, hipStream_t s);
// Same function, encoder 0 as one Winograd F(4,3) tile over the 4 frames, loop-structured code (kernel_front_f43.hip);
// `wfront` points to the F(4,3) image (layout.hpp w4_* units).  The product's fp32 frontend.
template <typename PcmT>
hipError_t launch_front_f43(int sr, const FrontArgs &a, hipStream_t s);
// The LATENCY form of the same kernel (kernel_front_lat.hip): one workgroup = 4 waves = ONE tile, every layer's output rows
// split over the waves; bit-identical results.  For launches of a few hundred tiles (one step of a stream pool, a B = 1 call).
template <typename PcmT>
hipError_t launch_front_lat(int sr, const FrontArgs &a, hipStream_t s);
// ONE step (nt == 1) with the LSTM cell and the head fused behind the latency frontend: no gx round trip, no second kernel.  The
// workgroup of a tile applies W_hh (image `whh_lat`: gate by gate in W_ih's block order) to h_{t-1}, exchanges the four gates through
// LDS, updates (h, c) in `state` in place and writes the tile's 16 probabilities.  Bit-identical to front + rec_kernel.
struct CellArgs {
    const float *whh_lat;    // [gate 4][kg 8][row block 8][lane 64][4]
    float *state;            // [2][B][128] in/out
    float *probs;            // [B][ldp], this step's column is t0
    long ldp;
    const uint8_t *present;  // [B] or null (= all): rows with present[b] == 0 have NO chunk this tick -- their (h, c) and their
                             // probability slot are not written (the carry pass of kernel_present.hip finishes the row)
};
template <typename PcmT>
hipError_t launch_step_lat(int sr, const FrontArgs &a, const CellArgs &c, hipStream_t s);
// The same ONE step with one workgroup per STREAM and every sum formed on the VALU in the MFMA program's order (kernel_step_one.hip):
// identical bits, a third of the time for a handful of streams (a B = 1 model call).  launch_front_one: the frontend half alone (gx in
// the fragment layout), for the bit-identity tests.
template <typename PcmT>
hipError_t launch_step_one(int sr, const FrontArgs &a, const CellArgs &c, hipStream_t s);
template <typename PcmT>
hipError_t launch_front_one(int sr, const FrontArgs &a, hipStream_t s);
// Same function, encoder 0 as two Winograd F(2,3) tiles over the frame pairs, straight-line code (kernel_front_wino.hip);
// `wfront` points to the F(2,3) image (layout.hpp w_* units).  A/B form, test builds only (VAD_AB; option enc0=winograd2).
template <typename PcmT>
hipError_t launch_front_wino(int sr, const FrontArgs &a, hipStream_t s);

// Recurrence: persistent over the slab's time steps; W_hh pinned in VGPRs, h exchanged through
// LDS, LSTM pointwise + head fused.  One workgroup (8 waves) per 16 streams.
struct RecArgs {
    const float *whh;        // packed recurrent image
    const float *tables;
    const float *gx;
    float *state;            // [2][B][128] in/out
    float *probs;            // [B][ldp]
    long ldp, t0, nt;
    int B;
    const uint8_t *present;  // [B] or null (= all); one-step calls only: an absent row's (h, c) and probability are not written
};
hipError_t launch_rec(int sr, const RecArgs &a, hipStream_t s);
// Live streams that have no chunk this tick (vad_step_present): behind the step kernels, for every row with present[b] == 0 the
// context is carried over unchanged, ctx_out[b] = ctx_in[b] (the frontend wrote the tail of whatever the row's PCM slot held), and
// the probability slot gets the sentinel VAD_PROB_ABSENT.  The step kernels themselves left the row's (h, c) unwritten.
hipError_t launch_carry_absent(const uint8_t *present, const float *ctx_in, float *ctx_out, int C, float *probs, long ldp, int B,
                               hipStream_t s);
// A compact tick of the pump (vad_pump_submit_compact): row pos[b] of `src` (the delivering streams' chunks back to back, row_bytes each,
// a multiple of 16) -> row b of `dst` for every b with present[b] != 0; rows of absent streams are not touched.  HBM to HBM.
hipError_t launch_expand_rows(const uint8_t *present, const int32_t *pos, const uint8_t *src, void *dst, long row_bytes, int B, hipStream_t s);
// A packet tick of the pump (vad_pump_submit_packets): table[i] = {stream b, sample offset into `pkt` (a multiple of 8), len (1 ... N),
// pending c (0 ... N - 1)}, at most one row per stream.  carry [streams][N] int16 holds each stream's pending samples (in place).  c + len
// >= N: row b of `batch` <- carry[b][0:c] ++ pkt[off:off + N - c], carry[b] <- the rest of the packet; otherwise carry[b][c:c + len] <-
// the packet and row b of `batch` is not touched.  N <= 512.  HBM to HBM.
hipError_t launch_assemble_packets(const int32_t *table, long n_rows, const int16_t *pkt, int16_t *carry, int16_t *batch, int N, hipStream_t s);
// The same for a tick with G.711 rows (vad_pump_submit_coded_packets): table[i] = {stream b, BYTE offset into `pkt` (a multiple of 16),
// len | codec << kCodecShift (codec VAD_PCM_S16 / _ULAW / _ALAW), pending c}; a G.711 row is expanded to int16 (g711_to_s16) on its way
// into the carry / the batch row.  Only ticks with at least one G.711 row take this kernel.
constexpr int kCodecShift = 16;
hipError_t launch_assemble_coded_packets(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int N,
                                         hipStream_t s);
// The same for a tick with at least one DVI4 row (codec VAD_PCM_DVI4: a 4-byte header {predict, index}, then len / 2 bytes of 4-bit
// codes, len even): that row is decoded (adpcm.hpp: two wave scans, the values of vad_adpcm_expand) on its way into the carry / the
// batch row; S16 and G.711 rows of the tick move as in launch_assemble_coded_packets.  Only ticks with a DVI4 row take this kernel.
hipError_t launch_assemble_adpcm_packets(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int N,
                                         hipStream_t s);
// A burst tick of the pump (vad_pump_submit_burst): a stream may have several rows and a row may be longer than N.  The table's rows are
// GROUPED BY STREAM, a stream's rows in arrival order: table[i] = {stream b, BYTE offset into `pkt` (a multiple of 16), len | codec <<
// kCodecShift, w}, w = pending c | k << kCodecShift on the first row of a stream (k = (c + the stream's lengths) / N chunks complete,
// k <= max_chunks) and < 0 on its other rows.  The work unit is the stream: carry[b][0:c] ++ row ++ row ... is cut into chunks of N;
// chunk 0 -> row b of `batch`, chunk j >= 1 -> row b of more[j - 1] (`more` = [max_chunks - 1][streams][N]), the remainder -> carry[b]
// (in place).  N <= 512, a multiple of 16.  adpcm: the tick has a DVI4 row (decoded in pieces of N samples, the decoder's state carried
// from piece to piece) and takes the kernel's ADPCM form; without one it takes the form it always took.
hipError_t launch_assemble_burst(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int16_t *more,
                                 int max_chunks, int streams, int N, bool adpcm, hipStream_t s);
// The flag rows of a burst tick's sub-steps 1 ... steps - 1: the tick's flag row holds k[b] (0 for a stream that completes no chunk),
// flags[(j - 1) * ld + b] = k[b] > j.
hipError_t launch_burst_flags(const uint8_t *k_of_stream, uint8_t *flags, long ld, int steps, int streams, hipStream_t s);
// A wide packet tick of the pump (vad_pump_submit_wide_packets): int16 rows sampled at step x 16 kHz, decimated to 16 kHz on their way
// into the carry / the batch row.  table[i] = {stream b, BYTE offset into `pkt` (a multiple of 16), len | step << kCodecShift | k0 <<
// kCombShift, pending c}: len = 1 ... step * N INPUT samples, step = 1 ... kMaxWideStep, k0 = comb_first(step, the stream's phase) = the
// row's first kept sample.  The row's kept samples pkt[k0], pkt[k0 + step], ... (comb_kept of them, <= N) are what assemble_packets'
// packet is: appended to carry[b][0:c], a chunk leaves when c + kept >= N.  At most one row per stream.  N <= 512.
constexpr int kCombShift = kCodecShift + 4;
constexpr int kMaxWideStep = 3;
hipError_t launch_assemble_wide_packets(const int32_t *table, long n_rows, const uint8_t *pkt, int16_t *carry, int16_t *batch, int N,
                                        hipStream_t s);
// Snapshot and restore of the pump's streams (vad_pump_export_streams* / vad_pump_import_streams; kernel_snapshot.hip).
// A RECORD of `records` (the blob's record layout) is the info block (32 bytes, the host's), h[128], c[128], ctx[C] (float) and int16
// pending[N]: 32 + 4 * (256 + C) + 2 * N bytes.  With a `tail` (blob versions 2 and 3) it goes on with the 32 bytes of vad_resample_info
// (the host's), float carry[N], int16 history[kSnapHistory] and tail->extra_bytes more of the host's (a multiple of 16; version 3: the 32
// bytes of vad_tape_info).
// The TABLE has one int4 per record, table[i] = {slot b, its part k, pending c (0 ... N - 1), record r}, and with a tail a second one
// behind it, {fp32 pending c (0 ... N - 1), H (0 ... hist_ld and kSnapHistory), bound 0 / 1, 0}; all range-checked by the host.
// parts[k] = part k's state block [2][n][128] and its first slot; `ctx` is the context buffer the pump's next tick reads.
// gather: record r <- zeros for the host's bytes, h, c, ctx[b], carry[b][0:c] ++ zeros and, of a bound stream, fcarry[b][0:c] ++ zeros,
// hist[b][0:H] ++ zeros (an unbound stream's tail: zeros).  scatter: the reverse -- the host's bytes are skipped, the carry row gets the
// record's first c samples ++ zeros, a bound record writes fcarry[b][0:N] = its first c floats ++ zeros and hist[b][0:hist_ld] = its first
// H samples ++ zeros, an unbound record leaves both rows alone.  fcarry: [streams][N] float, hist: [streams][hist_ld] int16, hist_ld a
// multiple of 8 (the pump's own pitch: the record's is always kSnapHistory); both null on a pump without the resampled route, whose
// table may hold no bound entry.  tail == nullptr (version 1): one table entry per record, neither buffer is known.  HBM to HBM.
struct SnapPart {
    float *state;
    int32_t lo, n;
};
struct SnapTail {
    float *fcarry;
    int16_t *hist;
    int hist_ld, extra_bytes;
};
constexpr int kSnapHistory = 160;            // == kResampleMaxTaps: H = K - 1 of every served pair fits
hipError_t launch_snapshot_gather(const int32_t *table, long n, const SnapPart *parts, const float *ctx, const int16_t *carry, int N, int C,
                                  uint8_t *records, hipStream_t s, const SnapTail *tail = nullptr);
hipError_t launch_snapshot_scatter(const int32_t *table, long n, const SnapPart *parts, float *ctx, int16_t *carry, int N, int C,
                                   const uint8_t *records, hipStream_t s, const SnapTail *tail = nullptr);
// Blob version 3 (vad_pump_export_streams_v3): the RUNS of the pump's tape (kernel_tape.hip) that a snapshot carries.  runs[i] = {slot b,
// n whole chunks, the first of them (a chunk number of the stream's clock, >= 0), where the run starts in `packed` (in chunks)}, all
// range-checked by the host: n <= chunks, slot b inside the tape, [at, at + n) inside `packed`.  gather: packed[at + k] <- tape[b][(first
// + k) % chunks]; scatter: the reverse, into the ring of a tape of `chunks` chunks (the destination's own).  elem: 2 (int16) or 4
// (float); tape and packed are 16-byte aligned and N % 8 == 0, so every row is whole 16-byte vectors on both sides.  HBM to HBM.
struct SnapRun {
    int32_t slot, n;
    int64_t first, at;
    int64_t pad;
};
hipError_t launch_snapshot_tape(bool scatter, const SnapRun *runs, long n_runs, long max_n, void *tape, int chunks, int N, int elem, void *packed,
                                hipStream_t s);

// The comb of the reference's decimation x[::step] (src/silero_vad/utils_vad.py:39-42) over a stream that arrives in pieces: input sample g
// of the stream is kept iff g % step == 0; `phase` = (samples that came before the piece) % step.  The one definition the pump's
// assembly kernel (kernel_present.hip), its host bookkeeping and the host export vad_decimate (pump.hip) share.
__host__ __device__ inline int comb_first(int step, int phase) { return phase ? step - phase : 0; }        // the piece's first kept sample
__host__ __device__ inline int comb_kept(int step, int k0, int len) { return len > k0 ? (len - k0 + step - 1) / step : 0; }

// ITU-T G.711 code -> 16-bit linear PCM, the values of Python's audioop.ulaw2lin / alaw2lin(x, 2).  The one definition the pump's
// assembly kernel (kernel_present.hip) and the host export vad_g711_expand (pump.hip) share.
__host__ __device__ inline int16_t ulaw_to_s16(uint8_t code) {
    const unsigned u = ~code & 0xffu;                                        // sign, 3-bit exponent, 4-bit mantissa, sent inverted
    const int t = (int)((((u & 0x0fu) << 3) + 0x84u) << ((u & 0x70u) >> 4));
    return (int16_t)((u & 0x80u) ? 0x84 - t : t - 0x84);
}
__host__ __device__ inline int16_t alaw_to_s16(uint8_t code) {
    const unsigned a = code ^ 0x55u;                                         // sign, 3-bit segment, 4-bit mantissa, even bits inverted
    const unsigned seg = (a & 0x70u) >> 4;
    const int m = (int)((a & 0x0fu) << 4);
    const int t = seg == 0 ? m + 8 : (m + 0x108) << (seg - 1);
    return (int16_t)((a & 0x80u) ? t : -t);
}
__host__ __device__ inline int16_t g711_to_s16(int codec, uint8_t code) {
    return codec == VAD_PCM_ULAW ? ulaw_to_s16(code) : alaw_to_s16(code);
}
// The same recurrence, bit for bit, for at most kRecSmallMaxB streams (1, 2 or 4 per workgroup): W_hh * h as matrix-vector products on the VALU (kernel_rec_small.hip);
// `whh` points at the row image (layout.hpp "whh_rows").
constexpr int kRecSmallMaxB = 1024;
hipError_t launch_rec_small(int sr, const RecArgs &a, hipStream_t s);
// The throughput frontend with every matrix product as exact bf16 x 9 piece products on the bf16 matrix pipe (kernel_front_b9.hip);
// `a.wfront` points at the three-piece image (layout.hpp "bf16 x 9 frontend image").  Same gx layout as launch_front_f43.
template <typename PcmT>
hipError_t launch_front_b9(int sr, const FrontArgs &a, hipStream_t s);
// The same recurrence with W_hh * h as exact bf16 x 9 piece products on the bf16 matrix pipe (kernel_rec_b9.hip); `whh` points
// to the three-piece image (layout.hpp "bf16 x 9 recurrent image").  Option "rec" = "bf16x9".
hipError_t launch_rec_b9(int sr, const RecArgs &a, hipStream_t s);

// Ingest (kernel_ingest.hip): rows[i].len elements (esz bytes each) at rows[i].ptr -- PINNED host memory, or device memory --
// -> dst[i][0 .. width), zero padded.  `rows` itself is read by the kernel (pinned or device memory).
struct RowDesc {
    const void *ptr;
    long len;
};
hipError_t launch_gather_rows(const RowDesc *rows, long n, long width, int esz, void *dst, bool rows_on_device, hipStream_t s);
// The same into an int16 batch from rows that may be G.711 (vad_upload_rows_coded): rows[i].len = samples | codec << kRowCodecShift,
// codec VAD_PCM_S16 (2 bytes a sample at an even address) or VAD_PCM_ULAW / _ALAW (1 byte a sample at ANY address, expanded by
// g711_to_s16 on the way); dst[i][0 .. width) int16, zero padded behind the row's last sample; width a multiple of 8.
constexpr int kRowCodecShift = 56;
hipError_t launch_gather_expand_rows(const RowDesc *rows, long n, long width, void *dst_i16, bool rows_on_device, hipStream_t s);
// The same over SOURCES of one or two interleaved channels (vad_upload_rows_channels): src[i].tag = frames | channels << kRowChanShift
// | codec << kRowCodecShift; channel c of source i becomes batch row src[i].dst[c] of dst[n_dst][width] (-1: not wanted), de-interleaved,
// expanded if G.711 and zero padded behind its last frame; batch rows nobody names are not written.  frame_bytes: the most bytes a frame
// of any source of the table has (1 ... 4), which sizes the launch.
constexpr int kRowChanShift = 48;
struct ChanRowDesc {
    const void *ptr;
    long tag;
    int32_t dst[2];
    int32_t pad[2];                  // 32 bytes: an entry never straddles a 64-byte line of the pinned table
};
hipError_t launch_gather_channels(const ChanRowDesc *src, long n, long width, int frame_bytes, void *dst_i16, bool rows_on_device,
                                  hipStream_t s);

// Resampling to the net's rate (kernel_resample.hip; the function, the table and the kernel's shape are described there).
constexpr int kResampleTile = 1024;          // outputs of one row a workgroup makes
constexpr int kResampleMaxRatio = 1024;      // caps of the pairs served (vad_resample_geometry): O = src / gcd and N = dst / gcd ...
constexpr int kResampleMaxTaps = 160;        // ... and K, the taps of a phase's live run
struct ResampleGeom {
    int O, N, W, K;
    int dlo, dhi;                            // min / max over the phases of first[j] - floor(j O / N)
    int span;                                // floats of LDS a tile stages at most
};
struct ResampleHostTable {                   // the one source of the table: taps[N][K] (a shorter run is followed by 0.0f), first[N]
    ResampleGeom g;
    std::vector<float> taps;
    std::vector<int32_t> first;
    // the STREAMING rule (vad_resample_stream_*): end[j] = first[j] - W + K, the inputs a stream must have received before output j of
    // period 0 is emitted (output q N + j: q O + end[j]).  Filled only when the rule is a count -- end[] non-decreasing and end[N - 1] <=
    // end[0] + O, so that the emitted outputs are always a prefix --; empty otherwise, and the pair then has no streaming form.
    std::vector<int32_t> end;
    int H = 0;                               // input samples of history a stream keeps: K - 1 (include/silero_vad_hip.h has the derivation)
};
// ready(g): the outputs a stream that has received g >= 0 inputs has emitted (t.end not empty).  64-bit throughout.
long resample_stream_ready(const ResampleHostTable &t, long g);
std::shared_ptr<const ResampleHostTable> resample_table(int src, int dst);      // null: the pair is not served; built once per process
struct ResampleDeviceTable {
    ResampleGeom g;
    float *taps;                             // TRANSPOSED, [K][N]: lanes of consecutive phases read consecutive floats
    int32_t *first;
};
// dst[r][m] = output m of row r for m < ceil(N lens[r] / O), 0.0f from there to width_out; pcm[n][ld] of esz 2 (int16, / 32768) or 4
// (float32); lens: device-visible.  Input at and past lens[r] (clamped to ld) counts as zero whatever the batch holds.
hipError_t launch_resample_rows(const ResampleDeviceTable &t, const void *pcm, int esz, long ld, const long *lens, long n, long width_out,
                                float *dst, long ldd, hipStream_t s);
// engine.hip: the pair's device table, made on first use and shared by the engine and its clones (what vad_resample_reserve puts there)
int engine_resample_table(vad_engine *e, int src, int dst, ResampleDeviceTable *out);

// A RESAMPLED packet tick of the pump (vad_pump_submit_resampled_packets; kernel_present.hip assemble_resampled_packets): int16 rows at
// one of up to kMaxPumpRates source rates, brought to the net's rate by the streaming form of the filter above on their way into the
// stream's fp32 carry / fp32 batch row.  The row table has kResampleRowWords int32 per row, every index computed and range-checked by
// the host: {stream b, BYTE offset into `pkt` (a multiple of 16; VAD_ROW_SILENT: zeros), len | rate << kResampleRateShift, fp32 pending
// c, base, j0, n_out, 0}.  The wave stages hist[b][0:H] ++ the row's len samples as floats in[0 : H + len); output i < n_out of the row
// is phase j = (j0 + i) % N of period dq = (j0 + i) / N: sum_k taps[k][j] in[base + dq O + first[j] + k], fmaf in tap order from 0.0f --
// the expression of resample_rows_kernel.  carry[b][0:c] ++ the outputs: c + n_out < 2 chunk; when they reach `chunk` the first `chunk`
// become row b of `batch` and the rest the new carry.  hist[b] <- the last H staged samples.  hist: [streams][hist_ld] int16, carry and
// batch: [streams][chunk] float.  max_len: the longest row the table may hold (sizes the LDS: (hist_ld + max_len + 2 chunk) floats).
constexpr int kMaxPumpRates = 4;
constexpr int kResampleRowWords = 8;
constexpr int kResampleRateShift = 24;
struct PumpRates {
    const float *taps[kMaxPumpRates];        // TRANSPOSED, [K][N]
    const int32_t *first[kMaxPumpRates];
    int O[kMaxPumpRates], N[kMaxPumpRates], K[kMaxPumpRates], H[kMaxPumpRates];
};
hipError_t launch_assemble_resampled_packets(const int32_t *table, long n_rows, const uint8_t *pkt, const PumpRates &rates, int16_t *hist,
                                             int hist_ld, int max_len, float *carry, float *batch, int chunk, hipStream_t s);

// Segmenter on the device (kernel_scan.hip): lane i scans probs[i * ldp ...] (or probs[row_off[i] ...] if row_off is
// not null), n_chunks[i] entries (or n_chunks_all if n_chunks is null), writes its segments to out[i * cap ...] and
// their number (may exceed cap) to counts[i].
hipError_t launch_scan(const float *probs, long ldp, const long *row_off, long n_streams, const long *n_chunks, long n_chunks_all,
                       const long *audio_len, const vad_segment_params &p, vad_segment *out, long cap, long *counts,
                       hipStream_t s);

// The audio inside (invert 0) or outside (invert 1) every row's segments, packed (kernel_collect.hip's two phases; the parts are
// collector.hpp).  pcm[n_rows][ld] of esz 2 | 4, 16 kHz sample s of a row at element s * step; segs[n_rows][cap] / counts[] as
// launch_scan left them, cap <= kCollectMaxCap (the gather keeps a row's prefix of part lengths in LDS).
//   launch_count_kept        kept[i] = samples row i keeps, -1 where counts[i] > cap
//   launch_collect_segments  row i's kept[i] samples to out + out_offset[i] (elements); nothing else is written
constexpr long kCollectMaxCap = 512;
hipError_t launch_count_kept(long ld, int step, long n_rows, const long *audio_len, const vad_segment *segs, long cap, const long *counts,
                             int invert, long *kept, hipStream_t s);
hipError_t launch_collect_segments(const void *pcm, int esz, long ld, int step, long n_rows, const long *audio_len, const vad_segment *segs,
                                   long cap, const long *counts, int invert, const long *kept, const long *out_offset, void *out,
                                   hipStream_t s);

// The pump's tape (kernel_tape.hip; the window rule and the ring's addressing are tape.hpp).  tape[streams][chunks][N] int16 and
// clock[streams][2] int64 = {count, floor} are device memory, rows[streams][N] the batch rows of one step, flags[streams] its flag row or
// nullptr; N is 256 or 512, every row 16-byte aligned.
//   launch_tape_rows    stream b with flags == nullptr || flags[b]: rows[b] -> tape[b][count % chunks], count += 1
//   launch_tape_gather  request i's `count` samples from sample `first` of stream `stream`'s clock to out + out_offset (elements); the
//                       caller has confined every request to its stream's window (0 <= first, count <= max_count <= chunks * N);
//                       nothing else is written
struct TapeRequest {
    int64_t stream, first, count, out_offset;
};
hipError_t launch_tape_rows(const int16_t *rows, const uint8_t *flags, int16_t *tape, int64_t *clock, int chunks, int streams, int N,
                            hipStream_t s);
hipError_t launch_tape_gather(const TapeRequest *req, long n_req, long max_count, const int16_t *tape, int chunks, int N, int16_t *out,
                              hipStream_t s);
// The fp32 tape (vad_pump_set_tape_f32): tape[streams][chunks][N] float, the same clock, the same requests ("sample" = one float).  Its
// rows come from an int16 batch -- taped as load_pcm gives them, (float)x * (1.0f / 32768.0f), exact -- or, on a resampled tick, from
// the fp32 batch, bit for bit.
hipError_t launch_tape_rows(const int16_t *rows, const uint8_t *flags, float *tape, int64_t *clock, int chunks, int streams, int N,
                            hipStream_t s);
hipError_t launch_tape_rows(const float *rows, const uint8_t *flags, float *tape, int64_t *clock, int chunks, int streams, int N,
                            hipStream_t s);
hipError_t launch_tape_gather(const TapeRequest *req, long n_req, long max_count, const float *tape, int chunks, int N, float *out,
                              hipStream_t s);

// The threshold sweep (kernel_sweep.hip; the cell is sweeper.hpp): row i's n_chunks[i] probabilities at probs + (row_off ? row_off[i]
// : i * ldp), its packed labels at labels + label_off[i]; tp / tn [n_rows][n_pairs], n_pos / n_valid [n_rows].  One wave per (row,
// 64 pairs): n_rows * ceil(n_pairs / 64) blocks, which the caller keeps below 2^31.
hipError_t launch_sweep(const float *probs, long ldp, const long *row_off, long n_rows, const long *n_chunks, const uint8_t *labels,
                        const long *label_off, const float *enter, const float *exit_, long n_pairs, int *tp, int *tn, int *n_pos,
                        int *n_valid, hipStream_t s);

// The validation scores (kernel_score.hip; the per-chunk rule is scorer.hpp).  launch_chunk_scores: rows addressed as launch_sweep's,
// row i's keys to keys + key_off[i]; one wave per row, n_rows < 2^31.  launch_auc_counts: out[3] = {U2, n_pos, n_neg} over the keys
// other than VAD_SCORE_KEY_NONE; workspace: auc_workspace_bytes(n) bytes, 16-byte aligned; 0 <= n < 2^31.
hipError_t launch_chunk_scores(const float *probs, long ldp, const long *row_off, long n_rows, const long *n_chunks, const uint8_t *labels,
                               const long *label_off, const long *key_off, uint32_t *keys, double *bce_pos, double *bce_neg, int *n_pos,
                               int *n_neg, int *n_bad, hipStream_t s);
size_t auc_workspace_bytes(long n);
hipError_t launch_auc_counts(const uint32_t *keys, long n, void *workspace, unsigned long long *out, hipStream_t s);

// test hook: y[i] = sigmoid (kind 0) / tanh (kind 1) of x[i] exactly as the recurrent kernels evaluate them (activations.hpp)
hipError_t launch_activation_probe(int kind, const float *x, float *y, long n, hipStream_t s);

// test hook: VALU-only spinner (kind 0 packed fp32, 1 scalar fp32), `blocks` one-wave workgroups
hipError_t launch_foreign_spin(float *sink, int blocks, long iters, int kind, hipStream_t s);

// gx (fragment order) -> row-major [B][T][512] for vad_debug_frontend
hipError_t launch_unpack_gx(const float *gx, float *out, int B, long T, hipStream_t s);


// Decoder training (kernel_train.hip; the rule and the workspace layout are trainer.hpp).  Every pointer is a device pointer; feat,
// w_ih and w_hh are 16-byte aligned, the workspace 256-byte aligned and train_layout(B, T).total bytes long.  Six launches, no
// synchronisation, no float atomics.
struct TrainArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w_out, *b_out;    // the parameters of THIS call
    const float *feat;                                         // [B][T][128]
    int B;
    long T;
    const long *n_chunks;                                      // [B], clamped to [0, T]
    const uint8_t *labels;                                     // [B][ldl]
    long ldl;
    const uint8_t *keep;                                       // [B][T][128] or nullptr
    float keep_scale, noise_loss;
    double denom;
    float *g_wih, *g_whh, *g_bih, *g_bhh, *g_wout, *g_bout;
    double *loss;
    float *probs;                                              // [B][T] or nullptr
    void *workspace;
};
hipError_t launch_decoder_grad(const TrainArgs &a, hipStream_t s);
// vad_encode_audio: gate rows 0 .. 127 of a slab of gx (fragment order, nt steps) -> feat[B][T][128] at steps t0 .. t0 + nt
hipError_t launch_unpack_feat(const float *gx, float *feat, int B, long T, long t0, long nt, hipStream_t s);

// Audio augmentation (kernel_augment.hip; the rule and the workspace layout are augment.hpp).  Every pointer is a device pointer; out
// is 16-byte aligned and ld_out a multiple of 4, the workspace 256-byte aligned and aug_layout(n, ld_out).total bytes long, n at
// most 65535.  One plan and one conversion launch, five launches per op position (a row without that op there leaves at once), one
// restoring launch; no synchronisation, no float atomics.
struct AugArgs {
    const void *pcm;                                           // [n][ld] int16 or float32
    int elem_size;
    long ld;
    const long *lens;                                          // [n]
    long n;
    const vad_augment_recipe *recipes;                         // [n]
    float *out;                                                // [n][ld_out]
    long ld_out;
    void *workspace;
    // vad_augment_rows_device_x (kernel_augment_x.hip): bank_len >= 0 admits FIR and ALIAS and queues three more launches per op
    // position; scratch is then a second [n][ld_out] float32 buffer, 16-byte aligned.  bank_len < 0: neither is read.
    const float *bank;                                         // [bank_len] or nullptr
    long bank_len;
    float *scratch;
};
hipError_t launch_augment(const AugArgs &a, hipStream_t s);
hipError_t launch_augment_x(const AugArgs &a, int pos, hipStream_t s);     // ALIAS, FIR and the copy back at one op position

// Resident training (kernel_trainset.hip; the rules are trainset.hpp).  Every pointer is a device pointer, element-aligned; the
// 16-byte path is chosen per vector from the addresses.  One launch, no synchronisation, no atomics.
struct TrainsetArgs {
    const void *arena;                                         // the corpus, int16 or float32
    int elem_size;
    const long *offs, *lens;                                   // [n_recordings], in elements
    const uint8_t *label_arena;
    const long *label_offs;                                    // [n_recordings]
    long n_recordings;
    const long *idx;                                           // [B]
    long B, max_samples, chunk;
    void *out_pcm;                                             // [B][ld] of the arena's type
    long ld;
    uint8_t *out_labels;                                       // [B][ldl]
    long ldl;
    long *out_lens, *out_n_chunks;                             // [B]
};
hipError_t launch_trainset_batch(const TrainsetArgs &a, hipStream_t s);
// torch.optim.Adam's step over the six decoder tensors: one launch, in front of it the state's reset when step == 1
hipError_t launch_decoder_adam(const vad_decoder_grads &p, const vad_decoder_params &g, const vad_decoder_grads &m, const vad_decoder_grads &v,
                               long step, double lr, double beta1, double beta2, double eps, hipStream_t s);

}  // namespace vad
