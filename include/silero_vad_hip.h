/*
 * silero_vad_hip.h -- C ABI of the MI355X (gfx950) Silero-VAD v6 inference engine.
 *
 * The reference has no C ABI for this path: its boundary is a duck-typed Python model object
 * (TorchScript VADRNNJITMerge, or OnnxWrapper over ONNX Runtime).  The entry points below are
 * what a binding for that object has to call; each cites the reference interface it replaces
 * (paths relative to the reference repo; "JIT!/" = TorchScript source inside
 * src/silero_vad/data/silero_vad.jit).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer marked "dev" is a DEVICE pointer on the
 *     engine's GPU (HBM-resident), everything else is host memory;
 *   - the caller owns all I/O buffers; the engine owns only its packed weights and scratch;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *     asynchronous with respect to the host unless stated otherwise;
 *   - one engine per GPU; an engine is not thread-safe (the reference model object is not
 *     either: src/silero_vad/utils_vad.py:51-92 mutates _state/_context per call);
 *   - the arithmetic is fp32 throughout, as in the reference: every contraction is a chain
 *     of v_mfma_f32_16x16x4_f32 (an fmaf chain, one rounding per product); what differs from the reference is WHICH
 *     fp32 sums are formed -- the STFT is a real FFT instead of the dense DFT-basis convolution, encoder 0 is evaluated in
 *     Winograd F(4,3) form (transformed weights, formed in double and rounded once) -- not their precision.  Agreement
 *     with the reference is therefore by tolerance, not bitwise: max |dp| 2e-6 on the reference's fixtures, <= 2e-5
 *     asserted on everything the GPU suite runs (the contract is 1e-4), final (h, c) within 1e-4;
 *   - sample rates 16000 (chunk N=512, context C=64) and 8000 (N=256, C=32); multiples of 16000 are decimated.
 */
#ifndef SILERO_VAD_HIP_H
#define SILERO_VAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vad_engine vad_engine;

enum vad_status {
    VAD_OK = 0,
    VAD_ERR_ARG = 1,        /* null pointer / negative size                                    */
    VAD_ERR_SAMPLE_RATE = 2,/* sr not in {8000, 16000}   (vad_annotator.py:95)                 */
    VAD_ERR_WEIGHTS = 3,    /* malformed weight container / missing tensor                     */
    VAD_ERR_NO_DEVICE = 4,  /* no HIP device, or not a gfx950 part                             */
    VAD_ERR_HIP = 5,        /* a HIP runtime call failed; see vad_last_error()                  */
    VAD_ERR_ALLOC = 6,      /* scratch allocation failed                                        */
    VAD_ERR_CAPTURE = 7,    /* scratch would have to grow while the stream is being captured    */
    VAD_ERR_OPTION = 8      /* unknown option name/value                                        */
};

/* ---- lifetime --------------------------------------------------------------------------------
 * Replaces load_silero_vad()/init_jit_model (src/silero_vad/model.py:6-36,
 * src/silero_vad/utils_vad.py:194-198): parses the SVADW001 weight container
 * (tools/export_weights.py; state_dict of silero_vad.jit), re-packs it into MFMA fragment order
 * and uploads it to `device`.                                                                  */
int  vad_create(const void *weights, size_t nbytes, int device, vad_engine **out);
void vad_destroy(vad_engine *e);
/* A second handle on the same GPU: shares the read-only weight images (no second copy) and starts with the same options,
 * owns its scratch.  An engine and its clones may have calls in flight on different streams at the same time (one engine
 * may not: its scratch is per call).  The reference gets concurrency by one model object per process
 * (examples/parallel_example.ipynb cell 5); inside one process on one GPU this is the equivalent.  Destroy every handle.
 * The calls may come from different host threads, one thread per handle at a time, on any streams (non-blocking ones included),
 * beside handles that are being created, grow their scratch or are destroyed: every handle returns the bits it returns alone
 * (tests/test_concurrency.py).  What the engine does not arrange: a hipGraph capture is a process-wide state of the runtime --
 * while one thread captures (global capture mode), allocating calls of other threads (vad_create / vad_clone / vad_pump_create, a
 * scratch growth) fail; capture while the other threads make no such call.
 * Host-only entry points across threads: vad_segment_probs, vad_iterator_feed, vad_g711_expand, vad_adpcm_expand, vad_deinterleave and vad_decimate are re-entrant (no shared state);
 * vad_stage_rows and vad_segment_probs_batch serialise themselves on the process-wide helper pool (tests/test_host_concurrency.py). */
int  vad_clone(const vad_engine *e, vad_engine **out);
const char *vad_strerror(int status);
const char *vad_last_error(const vad_engine *e);   /* detail text of the last failing call */
int  vad_device(const vad_engine *e);

/* Geometry of a sample rate (returns VAD_ERR_SAMPLE_RATE otherwise).
 * chunk: 512|256 (utils_vad.py:60), context: 64|32 (utils_vad.py:66).                           */
int  vad_geometry(int sr, int *chunk, int *context);

/* Options (strings so that bindings need no enum mirror):
 *   "impl"      = "mfma" (default, the product path) | "reference" (slow all-VALU kernels kept
 *                 as an on-device A/B for tests; never the default)
 *   "precision" = "fp32": the only arithmetic (accepted so that a binding may state it; anything else is VAD_ERR_OPTION)
 *   "gx_cap_mib"= cap, in MiB, of the engine's scratch for the LSTM input-gate pre-activations (default 6144);
 *                 a call whose B x T needs more is processed in time slabs, transparently
 *   "enc0"      = "winograd" (default; "winograd4" is a synonym): encoder 0 -- more than half of the frontend's matrix
 *                 work -- as ONE Winograd F(4,3) tile over the chunk's 4 STFT frames, 6 GEMMs instead of 10, all in fp32
 *                 (csrc/kernel_front_f43.hip).  The test build libsilero_vad_hip_ab.so (__graft_entry__.build, -DVAD_AB=1)
 *                 also accepts "winograd2" (two F(2,3) tiles, csrc/kernel_front_wino.hip) and "direct" (tap by tap,
 *                 csrc/kernel_front.hip: bitwise the plain fmaf chain over the taps) as A/B forms for the parity tests
 *   "rec"       = "fp32" (default) | "bf16x9": how the recurrence evaluates W_hh * h -- as the fp32 MFMA chain, or as the nine
 *                 exact products of three bf16 pieces per operand (x = p0 + p1 + p2 exactly) on the bf16 matrix pipe with fp32
 *                 accumulation (csrc/kernel_rec_b9.hip).  Not narrower than fp32 (no operand bit is dropped, every product is
 *                 exact), but a different summation: opt-in; measured against a float64 recurrence by the GPU suite
 *   "rec_form"  = "auto" (default) | "mfma": the fp32 recurrence has two forms with bit-identical results -- 16 streams per CU on the
 *                 matrix pipe (csrc/kernel_rec.hip: 4.3 us per step whatever the batch) and, for B <= 1024, W_hh h as fmaf chains on the
 *                 VALU in the MFMA chain's summation order, 1-4 streams per CU (csrc/kernel_rec_small.hip: 1.0-2.6 us per step; a file
 *                 at a time).  "mfma" forces the first (tests; callers that overlap several calls and want a call on few CUs)
 *   "front_mma" = "fp32" (default) | "bf16x9": the same for the frontend's matrix products (encoders 0-3 and W_ih): the fp32 MFMA
 *                 chain, or exact bf16 x 9 piece products (csrc/kernel_front_b9.hip; FFT, Winograd transforms, Nyquist update,
 *                 biases and ReLU stay the fp32 VALU code).  With "bf16x9" EVERY launch takes that kernel, whatever its size
 *                 (no latency form, no fused step: the arithmetic of a result must not depend on the batch it came in).
 *                 Opt-in; 10-20 % faster than the fp32 frontend, not more
 *   "front"     = "auto" (default) | "throughput" | "latency": the frontend has two forms with bit-identical results --
 *                 one wave per 16-chunk tile (csrc/kernel_front_f43.hip: tens of thousands of tiles per launch) and one
 *                 4-wave workgroup per tile (csrc/kernel_front_lat.hip: a stream pool's step, a B = 1 call); "auto" takes
 *                 the latency form for launches of at most 768 tiles.  The other two values force one form (tests)
 *   "fuse_step" = "1" (default) | "0": a ONE-step call that takes the latency form (vad_step of a stream pool, a B = 1 call)
 *                 runs the LSTM cell and the head inside the frontend's kernel -- no second launch, no trip of the gate
 *                 pre-activations through HBM; bit-identical to the two-kernel path ("0": force that, A/B for tests)
 *   "exact_transitions" = "1" (default) | "0": a chunk that holds an EXACTLY silent STFT frame (every sample zero: a muted source, a DTX
 *                 gap, the zero padding behind a recording's end) beside a frame that is not silent gets its gate pre-activations from a
 *                 double-precision evaluation of the frontend (csrc/exact_front.hpp: the reference's definition, its own fp32 DFT basis,
 *                 every sum in double, one rounding), because every one-accumulator fp32 summation is ill-conditioned exactly there
 *                 (carried (h, c) up to 1.2e-4 from float64 against <= 2e-5 on continuous audio; with the option 1e-5).  A pure function
 *                 of the chunk's own samples, identical bits on every route.  A chunk whose FOUR frames are silent takes the net's constant
 *                 for a chunk of zeros, evaluated the same way once (the chains make the same rounding error in every silent chunk and the
 *                 cell state integrates it: 4.6e-5 one chunk into a silence, 1e-5 with the constant).  "0": the fp32 chains everywhere,
 *                 "edges": without the constant (A/B for tests and studies).
 *                 fp32 frontend only (not with front_mma = bf16x9)
 *   "step_one"  = "auto" (default: 256, the number of CUs) | "0".."4096": a ONE-step call of at most this many streams (the B = 1
 *                 `model(chunk, sr)` of every unmodified caller; a tick of a small stream pool) takes one workgroup per STREAM
 *                 (csrc/kernel_step_one.hip: every sum of the step as an fmaf chain on the VALU in the MFMA program's summation order,
 *                 read from the same packed weight images -- bit-identical to the tile kernels; 25.0-26.5 us for 1..256 streams against
 *                 31.4-34.2 us, because no matrix instruction computes 16 columns for one stream and every stream has a CU to itself;
 *                 beyond one workgroup per CU the tile kernels win); "0": the 16-stream tile kernels for every batch (A/B for tests)
 *   "fused_decimation" = "1" (default) | "0": for sr = 32000 and 48000 the fp32 frontend reads every 2nd / 3rd sample
 *                 itself; "0" forces the separate decimation pass that the higher multiples of 16000 use (A/B for tests)
 *   "profile"   = "0" | "1"   record hipEvents around each kernel (vad_kernel_times)
 *   "trace_ptr" = device address (bring-up only): builds compiled with -DVAD_TRACE=1 write 16
 *                 int64 phase timestamps per frontend workgroup there; the one-stream step kernel leaves the shader clock of its
 *                 phase boundaries there in every build (tools/b1_phase_trace.py); "0" = off (default)  */
int  vad_set_option(vad_engine *e, const char *name, const char *value);

/* ---- the hot path ----------------------------------------------------------------------------
 * One step for B independent streams: the functional form of VADRNNJITMerge.forward
 * (JIT!/vad/model/vad_annotator.py:14-90) == the ONNX graph I/O used by OnnxWrapper.__call__
 * (src/silero_vad/utils_vad.py:57-92, session.run at :80-82):
 *     x1 = cat(ctx, pcm);  prob, state' = net(x1, state);  ctx' = x1[:, -C:]
 *   pcm    dev [B][N]   fp32 in [-1,1], row stride `ld` floats
 *   ctx    dev [B][C]   in/out  (zeros after a reset)
 *   state  dev [2][B][128] in/out  (h stacked on c; zeros after a reset)
 *   prob   dev [B]      out                                                                     */
int  vad_step(vad_engine *e, int sr, int B, const float *pcm, long ld, float *ctx, float *state,
              float *prob, void *stream);

/* The same step from HOST audio to HOST probabilities, the shape of the reference's streaming callers (host chunk in, probability out:
 * src/silero_vad/utils_vad.py:507-549 VADIterator; examples/cpp/silero-vad-onnx.cpp:103-142 feeds int16-derived chunks the same way):
 * one copy of the B chunks host -> dev_pcm, the step, one copy of the B probabilities dev_prob -> host_prob, all asynchronous on
 * `stream` (record an event behind the call and wait for it before reading host_prob).  May be issued inside a stream capture: the
 * three operations then become one hipGraph (what StreamPool replays per tick).
 *   host_pcm   host [B][N], PAGE-LOCKED; elem_size 2 = int16 (scaled by 1/32768 in the kernel's loads), 4 = fp32
 *   dev_pcm    dev  [B][N] of the same element type: staging the caller owns (16-byte aligned); or NULL: no copy -- the kernel reads
 *              host_pcm through the device's view of it (for a handful of streams: a B = 1 call is 2 KB)
 *   dev_prob   dev  [B], or NULL: the kernel then stores the probabilities straight into host_prob (no device copy, no D2H operation)
 *   host_prob  host [B], page-locked                                                                                            */
int  vad_step_host(vad_engine *e, int sr, int B, const void *host_pcm, size_t elem_size, void *dev_pcm, float *ctx, float *state,
                   float *dev_prob, float *host_prob, void *stream);

/* vad_step_host(dev_pcm = NULL, dev_prob = NULL) that RETURNS WHEN THE B PROBABILITIES ARE IN host_prob: the blocking call every
 * unmodified caller of the reference makes, `model(chunk, sr).item()` once per 32 ms (src/silero_vad/utils_vad.py:324-336
 * get_speech_timestamps, :528 VADIterator.__call__; examples/cpp/silero-vad-onnx.cpp:103-142 around session.Run).  The kernels store a
 * stream's probability as their last act, so the call waits for the B slots themselves to change (a bounded spin on the page-locked
 * memory; hipStreamSynchronize if they have not after 0.4 ms) instead of for the stream's completion signal.  ctx / state are device
 * buffers as in vad_step; later work on `stream` is ordered behind the step as usual.  A blocking call: not inside a stream capture
 * (capture vad_step_host).                                                                                                      */
int  vad_step_host_sync(vad_engine *e, int sr, int B, const void *host_pcm, size_t elem_size, float *ctx, float *state, float *host_prob,
                        void *stream);

/* vad_step with the two contexts apart and either PCM type, all on the device: reads ctx_in, writes the next context to ctx_out
 * (a second buffer: the kernel may not write where other waves still read), so that a caller that alternates two context buffers
 * pays no device-to-device copy per step.  The functional form once more -- the ONNX graph's inputs and outputs are distinct
 * tensors too (src/silero_vad/utils_vad.py:80-83: `state` in, `stateN` out).
 *   pcm  dev [B][N], elem_size 2 = int16 (scaled by 1/32768 in the kernel's loads) | 4 = fp32, row stride `ld` elements      */
int  vad_step_split(vad_engine *e, int sr, int B, const void *pcm, size_t elem_size, long ld, const float *ctx_in, float *ctx_out,
                    float *state, float *prob, void *stream);

/* The step for LIVE streams that do not all have a chunk this tick.  In the reference a stream's (h, c) and context change only when
 * that stream's own caller calls the model -- one call per chunk that arrived (src/silero_vad/utils_vad.py:507-549 VADIterator.__call__;
 * the model object replaces _state / _context inside that call and nowhere else, JIT!/vad/model/vad_annotator.py:72,86-87; the native
 * loop around session.run: examples/cpp/silero-vad-onnx.cpp:335-390) -- so a stream whose packet is late simply is not stepped.  In a
 * lock-step batch that is a per-row flag:
 *   present  dev [B] bytes (device memory, or page-locked host memory's device alias), or NULL = every row has a chunk.
 *            present[b] == 0: row b comes out of the call exactly as it went in -- (h, c) not written, its context carried over
 *            bit for bit (ctx_out[b] = ctx_in[b]), whatever its PCM row holds is ignored -- and prob[b] = VAD_PROB_ABSENT.
 *            The other rows' results do not depend on the flags (bit-identical to the call without them).
 *   ctx_out  a second buffer (as vad_step_split), or NULL / == ctx_in: in place (as vad_step)
 *   pcm      dev [B][N], elem_size 2 = int16 | 4 = fp32, row stride `ld` elements
 * With present == NULL this IS vad_step_split / vad_step: same kernels, same cost.  With flags it is one more small launch (the carry
 * of the absent rows' contexts, csrc/kernel_present.hip).                                                                       */
#define VAD_PROB_ABSENT (-1.0f)
int  vad_step_present(vad_engine *e, int sr, int B, const void *pcm, size_t elem_size, long ld, const float *ctx_in, float *ctx_out,
                      float *state, float *prob, const uint8_t *present, void *stream);
/* vad_step_host with the flags: host_present host [B] page-locked (NULL = all present: exactly vad_step_host), dev_present dev [B]
 * staging the caller owns; one more small H2D copy on `stream`.                                                                  */
int  vad_step_host_present(vad_engine *e, int sr, int B, const void *host_pcm, size_t elem_size, void *dev_pcm, float *ctx, float *state,
                           float *dev_prob, float *host_prob, const uint8_t *host_present, uint8_t *dev_present, void *stream);

/* T = ceil(L / N) lock-step steps for B streams: VADRNNJITMerge.audio_forward
 * (JIT!/vad/model/vad_annotator.py:128-156; ONNX twin utils_vad.py:94-110) with the carried
 * state made explicit (pass zeroed ctx/state for the reference's reset-then-run behaviour).
 * A last partial chunk is right-padded with zeros, as the reference does (:141-148).
 * `sr` may also be a multiple of 16000 (32000, 48000, ...): the input is then decimated to 16 kHz,
 * x[:, ::sr/16000] (no filter, first sample kept -- vad_annotator.py:104-112, utils_vad.py:39-42), on
 * the device -- for 32 and 48 kHz inside the frontend's own loads, without an extra pass over HBM -- and L / T
 * refer to the input / to ceil(ceil(L / k) / 512) chunks.
 *   pcm    dev [B][L]   row stride `ld`
 *   probs  dev [B][T]   row stride `ldp`                                                        */
int  vad_forward_audio(vad_engine *e, int sr, int B, long L, const float *pcm, long ld,
                       float *ctx, float *state, float *probs, long ldp, void *stream);

/* Same, 16-bit PCM in HBM; samples are scaled by 1/32768 on load, the convention of the
 * reference's non-Python clients (examples/cpp/wav.h:113-118, examples/onnx_sequence/run.py:119). */
int  vad_forward_audio_i16(vad_engine *e, int sr, int B, long L, const int16_t *pcm, long ld,
                           float *ctx, float *state, float *probs, long ldp, void *stream);

/* Pre-size the engine-owned scratch for (sr, B, T) so that later calls allocate nothing (needed
 * before capturing vad_step/vad_forward_audio into a hipGraph; T counts chunks at the net's rate, sr may be a
 * multiple of 16000 -- the worst-case tail copy of a 48 kHz fp32 input is included).  Synchronous.                 */
int  vad_reserve(vad_engine *e, int sr, int B, long T);
size_t vad_scratch_bytes(const vad_engine *e);
/* The engine's scratch only ever grows; when a later call (or vad_reserve) needs more than it has, the
 * buffers are freed and reallocated (synchronously, and never while a stream is being captured:
 * VAD_ERR_CAPTURE).  A hipGraph that captured vad_step / vad_forward_audio holds the OLD device addresses,
 * so it MUST be re-captured after such a growth: this counter changes exactly when that happened.
 * (silero_vad_amd/streams.py StreamPool checks it before every replay.)                               */
unsigned long vad_scratch_generation(const vad_engine *e);

/* With option profile=1 the engine brackets its kernels with hipEvents on the caller's stream
 * (no host synchronisation at record time).  This call waits for them and returns the GPU time in
 * ms SUMMED over all vad_step/vad_forward_audio calls since the previous query (`calls` of them):
 * front = framing + STFT + encoder + input-gate GEMM kernel, rec = LSTM recurrence + head kernel. */
int  vad_kernel_times(vad_engine *e, float *front_ms, float *rec_ms, long *calls);

/* ---- post-processing on the host ----------------------------------------------------------------
 * The hysteresis segmenter of get_speech_timestamps (src/silero_vad/utils_vad.py:338-450) as a
 * native routine (C++ twin in the reference: examples/cpp/silero-vad-onnx.cpp:196-389).
 * Field names and defaults are those of the Python signature (utils_vad.py:212-227).             */
typedef struct vad_segment_params {
    double threshold;                    /* 0.5   (double: Python compares in double)       */
    double neg_threshold;                /* < 0 => max(threshold - 0.15, 0.01)  (:342-343)  */
    int    sampling_rate;                /* 8000 | 16000 (already decimated)                */
    int    min_speech_duration_ms;       /* 250                                             */
    double max_speech_duration_s;        /* +inf                                            */
    int    min_silence_duration_ms;      /* 100                                             */
    int    speech_pad_ms;                /* 30                                              */
    int    min_silence_at_max_speech_ms; /* 98                                              */
    int    use_max_poss_sil_at_max_speech; /* 1                                             */
} vad_segment_params;

typedef struct vad_segment { int64_t start, end; } vad_segment;   /* sample indices */

void vad_segment_params_default(vad_segment_params *p, int sampling_rate);

/* probs[n] -> speech segments of an audio of `audio_len` samples.  Writes at most `cap`
 * segments to `out`; returns the number of segments found (may exceed cap), <0 on bad args.      */
long vad_segment_probs(const float *probs, long n, long audio_len, const vad_segment_params *p,
                       vad_segment *out, long cap);

/* The same scan for many independent streams (one row of probs per stream, row stride `ldp`,
 * n_chunks[i] valid entries, audio of audio_len[i] samples): what a corpus run does after
 * vad_forward_audio (the reference fans this out as one Python process per file,
 * examples/parallel_example.ipynb cells 5, 7).  Stream i's segments go to
 * out[i * cap_per_stream ...], their number (may exceed cap_per_stream) to counts[i].  Streams are
 * split over `threads` persistent host threads (<= 0: vad_host_threads()).  Returns the total number of
 * segments, <0 on bad arguments.                                                                */
long vad_segment_probs_batch(const float *probs, long ldp, long n_streams, const long *n_chunks,
                             const long *audio_len, const vad_segment_params *p, vad_segment *out,
                             long cap_per_stream, long *counts, int threads);

/* The same scan ON THE DEVICE, for probabilities that vad_forward_audio just left in HBM: one GPU lane per
 * stream, so that only the segment lists cross PCIe (16 B per segment) instead of every probability, and the host
 * does no per-chunk work (the reference does it in a Python loop per file: utils_vad.py:348-440).  All pointers
 * are DEVICE pointers except `p`.  n_chunks may be NULL: every stream then has n_chunks_all (<= ldp) entries.
 * row_offsets may be NULL: stream i's probabilities then start at probs[i * ldp]; otherwise at probs[row_offsets[i]]
 * (ragged rows packed back to back, as the continuous-refill scheduler leaves them).
 * Stream i's segments go to out[i * cap_per_stream ...], their number (may exceed cap_per_stream: grow and call
 * again) to counts[i].  Asynchronous on `stream`.  Same results as vad_segment_probs_batch, bit for bit (one
 * source, csrc/scanner.hpp).                                                                        */
int  vad_segment_probs_device(vad_engine *e, const float *probs, long ldp, const long *row_offsets, long n_streams,
                              const long *n_chunks, long n_chunks_all, const long *audio_len, const vad_segment_params *p,
                              vad_segment *out, long cap_per_stream, long *counts, void *stream);

/* ---- the audio the segments keep ----------------------------------------------------------------------------------------------
 * collect_chunks / drop_chunks (src/silero_vad/utils_vad.py:552-655) for every row of a batch that is still in HBM, right behind
 * vad_segment_probs_device: the samples inside (invert = 0) or outside (invert = 1, up to audio_len[i]) row i's segments, packed, so
 * that only the kept audio leaves the device -- or none of it, for a consumer on the same GPU.  All pointers are DEVICE pointers.
 * pcm[n_streams][ld] of elem_size 2 (int16) or 4 (float32) is the batch as vad_forward_audio[_i16] received it; it holds raw-rate
 * samples, 16 kHz sample s of row i is pcm[i * ld + s * step], step 1, 2 or 3 (16 / 32 / 48 kHz).  audio_len (16 kHz samples), segs,
 * cap_per_stream (<= 512) and counts are what the scan was given and wrote.  A segment is clamped to [0, audio_len[i]] and one with
 * end < start is empty; audio_len[i] itself is confined to the samples a row of ld elements holds.
 * Two phases, both asynchronous on `stream`:
 *   out == NULL  COUNT: kept[i] = the number of samples row i keeps; -1 for a row with counts[i] > cap_per_stream (its list is
 *                incomplete: rescan it with room, or collect it on the host with vad_collect_segments).  pcm and out_offset are not read.
 *   out != NULL  GATHER: row i's kept[i] samples go to out + out_offset[i] (in elements).  The caller derives out_offset from kept --
 *                an exclusive sum of the kept counts, each rounded up to 16 bytes, keeps every row's start 16-byte aligned, which is
 *                what the kernel's vector stores want (any other offset is honoured element by element) -- and sizes out by it.
 *                Exactly kept[i] elements are written per row: the padding between rows and everything behind the last row is not
 *                touched.  Rows with kept[i] <= 0 write nothing.
 * Bit for bit what vad_collect_segments gives for each row.  VAD_ERR_ARG, before anything is queued: elem_size not 2 or 4, step not
 * 1 ... 3, invert not 0 or 1, a negative size, cap_per_stream above 512, a NULL audio_len / counts / kept (segs with a cap; pcm and
 * out_offset with out), pcm not aligned to its elements, out not 16-byte aligned.  A host-only engine: VAD_ERR_NO_DEVICE.          */
int  vad_collect_segments_device(vad_engine *e, const void *pcm, size_t elem_size, long ld, int step, long n_streams,
                                 const long *audio_len, const vad_segment *segs, long cap_per_stream, const long *counts,
                                 int invert, long *kept, const long *out_offset, void *out, void *stream);
/* host twin, one stream, re-entrant, no GPU: the same samples of pcm (a HOST pointer; sample s at element s * step) for n_segs
 * segments, in one pass.  Returns the number of samples the segments keep: they were written to out if out is given and cap (the
 * room of out, in samples) holds them; with out == NULL or a cap that is too small nothing is written and the number says what is
 * needed.  -VAD_ERR_ARG for a bad elem_size / step / invert, a negative size, NULL segs with n_segs > 0, NULL pcm with samples to copy. */
long vad_collect_segments(const void *pcm, size_t elem_size, int step, long audio_len, const vad_segment *segs, long n_segs,
                          int invert, void *out, long cap);

/* ---- the enter / exit threshold sweep ---------------------------------------------------------------------------------------------
 * What tuning/search_thresholds.py computes on a labelled validation corpus (calculate_best_thresholds, tuning/utils.py:326-356), as
 * integer counts: for every row i of probabilities and every threshold pair k the confusion counts of the hysteresis decision
 * against per-chunk labels.  The decision starts at 0; per chunk, in order: p >= enter[k] sets it, else p <= exit[k] clears it,
 * anything else (a NaN too) holds it; then tp += (decision && label == 1), tn += (!decision && label == 0).  labels are uint8: 0 not
 * speech, 1 speech, any other value (VAD_LABEL_IGNORE) a chunk that is not there -- skipped, decision untouched, nothing counted.
 * Any pair is accepted (exit >= enter is defined by the order of the two tests).  The comparisons are fp32: a caller with float64
 * thresholds rounds enter UP and exit DOWN to float32, which decides every float32 probability as the float64 comparison does.
 *
 * Row i's n_chunks[i] probabilities start at probs[i * ldp] (row_offsets NULL; n_chunks[i] <= ldp) or at probs[row_offsets[i]]; its
 * n_chunks[i] labels start at labels[label_offsets[i]], packed, no alignment required.  Nothing behind a row's n_chunks[i] entries is
 * read.  Outputs, int32: tp, tn [n_streams][n_pairs]; n_pos[i] = labels equal to 1, n_valid[i] = labels equal to 0 or 1 (accuracy is
 * (tp + tn) / n_valid; precision, recall and F1 follow from the same four numbers).  Exactly those cells are written.
 *
 * vad_threshold_counts_host: re-entrant, no GPU; rows are split over `threads` persistent host threads (<= 0: vad_host_threads()).
 * vad_threshold_counts_device: right behind vad_forward_audio, for probabilities that are still in HBM: ALL pointers are DEVICE
 * pointers, asynchronous on `stream`, allocates nothing, one wave per (row, 64 pairs) -- only the counts have to cross the link.
 * The two give the same counts, as integers (one source, csrc/sweeper.hpp).  VAD_ERR_ARG: a NULL pointer (with n_streams > 0; enter
 * and exit always), a negative size, n_pairs <= 0; on the host also a negative n_chunks[i] / offset or n_chunks[i] > ldp without
 * row_offsets; on the device probs not aligned to 4 bytes or n_streams * ceil(n_pairs / 64) >= 2^31.  A host-only engine:
 * VAD_ERR_NO_DEVICE.                                                                                                                */
#define VAD_LABEL_IGNORE 255
int  vad_threshold_counts_host(const float *probs, long ldp, const long *row_offsets, long n_streams, const long *n_chunks,
                               const uint8_t *labels, const long *label_offsets, const float *enter, const float *exit, long n_pairs,
                               int32_t *tp, int32_t *tn, int32_t *n_pos, int32_t *n_valid, int threads);
int  vad_threshold_counts_device(vad_engine *e, const float *probs, long ldp, const long *row_offsets, long n_streams,
                                 const long *n_chunks, const uint8_t *labels, const long *label_offsets, const float *enter,
                                 const float *exit, long n_pairs, int32_t *tp, int32_t *tn, int32_t *n_pos, int32_t *n_valid,
                                 void *stream);

/* ---- validation scores: masked BCE sums and the pooled ROC-AUC ---------------------------------------------------------------------
 * What the reference's validate() reports on a labelled validation set (tuning/utils.py:252-298): the BCE loss of the per-chunk
 * probabilities against the labels and roc_auc_score over every chunk of the set.  Two steps, each with a host twin.
 *
 * 1. The per-chunk rule (one source, csrc/scorer.hpp).  A chunk is VALID when its label is 0 or 1 and 0 <= p <= 1 (a NaN fails that;
 *    -0.0f passes and counts as +0.0f).  A label above 1 (VAD_LABEL_IGNORE) is a chunk that is not there.  A label of 0 / 1 with any
 *    other probability is BAD: counted in n_bad, in no sum, without a key.  A valid chunk's BCE term is nn.BCELoss's, the log taken
 *    in double: label 1: -max(log((double)p), -100); label 0: -max(log((double)(1.0f - p)), -100), the subtraction in fp32.  Its key
 *    is (v << 1) | label with v the bit pattern of p (v <= 0x3F800000, monotone in p); every other chunk's key is
 *    VAD_SCORE_KEY_NONE.
 *    Rows are addressed as in the threshold sweep (probs, ldp, row_offsets, n_chunks, labels, label_offsets); row i's keys go to
 *    keys[key_offsets[i] + t], t < n_chunks[i].  Outputs per row: bce_pos[i] / bce_neg[i] (double: the sums of the terms of the valid
 *    label-1 / label-0 chunks), n_pos[i], n_neg[i] (valid chunks by label), n_bad[i].  Exactly those cells are written; nothing behind
 *    a row's n_chunks[i] entries is read.  The sums are accumulated in double in an order that depends on the row alone: a row gives
 *    the same bits at any position of any batch, at any pitch and alignment.  Host and device give the same integers and keys; each
 *    device sum lies within (2 n + 8) * 2^-53 * sum of the host's (n = n_chunks[i]: two logs of at most 2 ulp, two summations of n
 *    non-negative terms).
 *    vad_chunk_scores_host: re-entrant, no GPU, rows over `threads` host threads (<= 0: vad_host_threads()).
 *    vad_chunk_scores_device: ALL pointers are DEVICE pointers, asynchronous on `stream`, allocates nothing, one wave per row.
 *    VAD_ERR_ARG: a NULL pointer (with n_streams > 0), a negative size; on the host also a negative n_chunks[i] / offset or
 *    n_chunks[i] > ldp without row_offsets; on the device probs not aligned to 4 bytes, bce_pos / bce_neg not to 8, or n_streams >=
 *    2^31.  A host-only engine: VAD_ERR_NO_DEVICE.
 *
 * 2. The pooled rank statistic over n keys, those equal to VAD_SCORE_KEY_NONE skipped: out[3] = { U2, n_pos, n_neg } with
 *    U2 = sum over the positive keys (low bit 1) of 2 * #{negative keys with a smaller v} + #{negative keys with an equal v}, so that
 *    U2 / (2 n_pos n_neg) is the Mann-Whitney statistic with ties at one half: what roc_auc_score returns.  Any other uint32 is a
 *    key (v = key >> 1); n < 2^31, so U2 fits 64 bits.
 *    vad_auc_counts_host: re-entrant, no GPU (a sort).  vad_auc_counts_device: keys, workspace and out are DEVICE pointers (out
 *    aligned to 8 bytes, workspace to 16), asynchronous on `stream`, allocates nothing: the caller provides a workspace of at least
 *    vad_auc_workspace_bytes(n) bytes (host-only call; 0 for an n outside [0, 2^31)); a smaller one is VAD_ERR_ARG with nothing
 *    written.  A counting scheme, no sort (csrc/kernel_score.hip).  Host and device give the same three integers.                   */
#define VAD_SCORE_KEY_NONE 0xFFFFFFFFu
int  vad_chunk_scores_host(const float *probs, long ldp, const long *row_offsets, long n_streams, const long *n_chunks,
                           const uint8_t *labels, const long *label_offsets, const long *key_offsets, uint32_t *keys, double *bce_pos,
                           double *bce_neg, int32_t *n_pos, int32_t *n_neg, int32_t *n_bad, int threads);
int  vad_chunk_scores_device(vad_engine *e, const float *probs, long ldp, const long *row_offsets, long n_streams,
                             const long *n_chunks, const uint8_t *labels, const long *label_offsets, const long *key_offsets,
                             uint32_t *keys, double *bce_pos, double *bce_neg, int32_t *n_pos, int32_t *n_neg, int32_t *n_bad,
                             void *stream);
size_t vad_auc_workspace_bytes(long n);
int  vad_auc_counts_host(const uint32_t *keys, long n, uint64_t *out);
int  vad_auc_counts_device(vad_engine *e, const uint32_t *keys, long n, void *workspace, size_t workspace_bytes, uint64_t *out,
                           void *stream);

/* The streaming caller, VADIterator.__call__ (src/silero_vad/utils_vad.py:507-549), for every slot of a lock-step batch: probs[n]
 * = this tick's probabilities (what vad_step left, copied to the host), active (may be NULL = all) marks the slots that carry a
 * live stream.  triggered / temp_end / current_sample are the iterator's per-stream state (zero after a reset, :500-503), updated
 * in place.  Writes at most `cap` events (slot order; kind 0 = {'start': sample}, 1 = {'end': sample}, the numbers the reference
 * iterator returns for that stream) and returns how many there were (may exceed cap; at most n), <0 on bad arguments.
 * threshold, min_silence_samples = sr * min_silence_duration_ms / 1000 and speech_pad_samples = sr * speech_pad_ms / 1000 are
 * doubles because the reference compares Python floats (:494-498).                                                          */
typedef struct vad_iter_event { int32_t slot; int32_t kind; int64_t sample; } vad_iter_event;
long vad_iterator_feed(const float *probs, const uint8_t *active, long n, int window, double threshold,
                       double min_silence_samples, double speech_pad_samples, uint8_t *triggered,
                       int64_t *temp_end, int64_t *current_sample, vad_iter_event *out, long cap);

/* ---- live streams: the pump --------------------------------------------------------------------------------------------
 * BASELINE configs[4] as one native object: `streams` live streams on one GPU advance in lock step, one tick = one 32 ms chunk of
 * every stream, host int16 audio in, VADIterator events out -- the loop the reference's native streaming clients run around
 * their runtime, one session.run per chunk with explicit state and the iterator logic inline
 * (examples/cpp/silero-vad-onnx.cpp:335-390; Python: src/silero_vad/utils_vad.py:507-549 VADIterator.__call__), for thousands of
 * streams at once.  The pump owns: a page-locked ingest ring [ring_slots][streams][N] int16 that the audio sources write
 * into, the device batch (three buffers), the carried (h, c) and context of every stream in HBM, the iterator state of every
 * stream, three HIP streams (copies of even / odd ticks, kernels) and the events that order them (csrc/pump.hip has the schedule:
 * tick t + 1's H2D runs beside tick t's kernel BY EVENT, nothing left to hardware-queue assignment).
 * One caller thread drives submit / poll; any thread may write a ring slot that is not in flight.                          */
typedef struct vad_pump vad_pump;
typedef struct vad_pump_params {
    int    sampling_rate;            /* 8000 | 16000                                                                         */
    int    streams;                  /* live streams (slots) on this GPU                                                     */
    int    parts;                    /* sub-batches per tick, each its own copy and kernel (<= 0: 1)                         */
    int    ring_slots;               /* ticks of audio the ingest ring holds (<= 0: 4; at least 2)                           */
    double threshold;                /* VADIterator arguments and defaults (utils_vad.py:477-498): 0.5                       */
    int    min_silence_duration_ms;  /* 100                                                                                  */
    int    speech_pad_ms;            /* 30                                                                                   */
} vad_pump_params;
typedef struct vad_pump_stats {
    long   ticks, events;
    double wall_ms;
    double tick_ms_p50, tick_ms_p95, tick_ms_max;     /* slot written -> its events on the host, per tick                    */
    double fill_ms_mean, submit_ms_mean, wait_ms_mean;/* host time per tick: writing the slot, issuing the tick, blocked     */
    int    fill_threads, depth;
    long   chunks;                                    /* chunks that were stepped (= ticks x streams unless streams were absent)  */
} vad_pump_stats;
enum { VAD_PUMP_IDLE = -1,   /* vad_pump_poll: nothing submitted                                                             */
       VAD_PUMP_BUSY = -2,   /* vad_pump_poll(block = 0): the oldest tick has not finished                                   */
       VAD_PUMP_ERROR = -3 };/* see vad_pump_last_error                                                                      */

void vad_pump_params_default(vad_pump_params *p, int sampling_rate, int streams);
/* The pump works on a clone of `e` (vad_clone): the caller's engine stays free for other calls, from another host thread too, and
 * several pumps may run beside each other, each driven by its own thread (tests/test_concurrency.py: two pumps, the engine they were
 * cloned from and further clones in flight together).  Every stream starts open, from zero state (VADIterator.reset_states,
 * utils_vad.py:500-505).                                                                                                    */
int  vad_pump_create(vad_engine *e, const vad_pump_params *p, vad_pump **out);
void vad_pump_destroy(vad_pump *p);
const char *vad_pump_last_error(const vad_pump *p);
int  vad_pump_geometry(const vad_pump *p, int *streams, int *chunk, int *ring_slots, int *parts);
/* Ring slot r: [streams][N] int16, page-locked; the sources write stream b's next chunk at slot + b * N.                   */
int16_t *vad_pump_slot(vad_pump *p, int r);
/* Start one tick over ring slot r: asynchronous (copies and kernels are queued; returns at once).  VAD_ERR_ARG while the slot's
 * previous tick is in flight.  Ticks execute in submission order.                                                          */
int  vad_pump_submit(vad_pump *p, int r);
/* The tick for live streams that do not all have a chunk (see vad_step_present): present = host [streams] bytes, 0 = stream b has no
 * chunk this tick -- its (h, c), context and iterator counters stay exactly as they are, its slot of vad_pump_probs holds
 * VAD_PROB_ABSENT, whatever its part of the ring slot holds is ignored; NULL = every stream has one (== vad_pump_submit, same copies,
 * same kernels).  Every ring slot has its own page-locked flag row, vad_pump_present(p, r), in front of its audio (flags and audio
 * cross the link in ONE copy): write the flags there and pass that pointer, or pass any host array (copied there).  A failure after
 * the tick's first operation was queued poisons the pump (every later call fails): the carried state is half-advanced.          */
uint8_t *vad_pump_present(vad_pump *p, int r);
int  vad_pump_submit_present(vad_pump *p, int r, const uint8_t *present);
/* The same tick from a COMPACT slot: the sources wrote only the chunks of the streams that deliver, back to back -- row i of
 * vad_pump_slot(p, r) is the chunk of the i-th stream (ascending) whose flag is set -- and only the flags, a position table and those
 * rows cross the link (one copy); a row-expansion pass on the device puts every chunk where the step kernels read it.  Results are
 * those of vad_pump_submit_present with the same flags, bit for bit; the link cost of a tick falls with the delivery rate.  present
 * must not be NULL.  Compact, masked and full ticks may be mixed freely.                                                         */
int  vad_pump_submit_compact(vad_pump *p, int r, const uint8_t *present);
/* A compact tick in ARRIVAL order -- what a receive path can fill without knowing who else will deliver: row i of vad_pump_slot(p, r)
 * is the chunk of stream stream_of_row[i], i < n_rows (receive threads append with one atomic row counter per slot); every other stream
 * is absent this tick.  A stream listed twice (two packets in one tick: keep the second for the next tick) or out of range is
 * VAD_ERR_ARG and nothing is queued.  n_rows == 0: a tick in which nobody delivers.  Results as vad_pump_submit_present with the same
 * set of streams, bit for bit.                                                                                                   */
int  vad_pump_submit_rows(vad_pump *p, int r, const int32_t *stream_of_row, long n_rows);
/* A PACKET tick -- what RTP / WebRTC / SIP receive paths deliver (10 / 20 / 30 ms frames, odd lengths after a loss): row i of slot r's
 * sample area (vad_pump_slot(p, r) seen as one flat int16 array of streams * N samples) holds len_of_row[i] samples of stream
 * stream_of_row[i], starting at sample offset off_of_row[i] -- a multiple of 8 samples, so that packets start on 16-byte boundaries
 * (receive threads append with one atomic sample counter rounded up to 8).  1 <= len <= N.  A stream's packets are appended to what
 * it has pending; a stream whose pending samples reach N this tick is stepped once on the first N of them and the rest stay pending;
 * every other stream is absent (vad_pump_submit_present semantics).  Probabilities, events, (h, c) and context are bit for bit those of
 * the same pump fed the concatenation of each stream's packets cut into N-sample chunks through vad_pump_submit_rows, each chunk at the
 * tick its last sample arrived (the reference's VADIterator on the concatenated audio, utils_vad.py:507-549).  A packet longer than N
 * (e.g. a 60 ms Opus frame at 16 kHz) is refused, not split: submit it over two ticks.  Invalid input is VAD_ERR_ARG and nothing is
 * queued: a stream out of range or listed twice, a length out of range, an offset that is misaligned or runs past the slot.  The chunk
 * routes (vad_pump_submit / _present / _compact / _rows) refuse (VAD_ERR_ARG, nothing queued) a chunk for a stream with samples
 * pending; vad_pump_open / vad_pump_close drop a stream's pending samples.  One copy per tick: row table, flags, packet samples.
 * SILENT rows -- time that passes without a payload.  A lost packet, a G.711 trunk with silence suppression (RFC 3389 comfort-noise
 * periods) and an Opus stream in DTX deliver nothing for 20 ms ... several seconds while the stream's clock runs.  A row whose offset
 * entry is VAD_ROW_SILENT stands for len_of_row[i] samples of digital silence (int16 0) of its stream and occupies NO bytes of the slot:
 * nothing is written on the host, nothing crosses the link for it (the tick's copy carries the row table, the flags and the payload
 * rows only; a tick of silent rows copies not one byte of the sample area).  It is a row in every other respect: appended behind the
 * stream's pending samples, it completes chunks, leaves a residue, counts as the stream's row of the tick ("listed twice") and towards
 * n_rows <= streams, and vad_pump_pending reports what it would after a payload row of that length; the alignment and fits-the-area
 * checks do not apply to it.  Every other negative offset stays VAD_ERR_ARG.  Probabilities, events, (h, c), context, pending samples
 * and comb phases are bit for bit those of the same pump fed, in the same row position and through the same route, a payload row of
 * len int16 zeros.  Here: off_of_row[i] == VAD_ROW_SILENT, 1 <= len <= N.
 * ABSENT against SILENT.  A stream whose packet is LATE is listed in no row: it is absent, and its (h, c), context, sample counter
 * and the iterator's silence timer freeze until the packet arrives.  A stream whose packet is LOST, or that is in DTX, is listed in a
 * silent row: its clock runs, min_silence_duration_ms counts on, the 'end' event of the segment before the gap is emitted during the
 * gap and every later vad_iter_event.sample stays true.  Only the caller's jitter buffer knows late from lost; the pump never fills a
 * gap by itself.                                                                                                                   */
#define VAD_ROW_SILENT (-1)
int  vad_pump_submit_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *off_of_row, const int32_t *len_of_row,
                             long n_rows);
/* Sample formats of a packet row: 16-bit linear PCM, ITU-T G.711 mu-law (PCMU) or A-law (PCMA), 1 byte per sample (SIP trunks,
 * telephony media streams: 8 kHz).                                                                                              */
enum { VAD_PCM_S16 = 0, VAD_PCM_ULAW = 1, VAD_PCM_ALAW = 2, VAD_PCM_DVI4 = 3 };
/* VAD_PCM_DVI4 (vad_pump_submit_coded_packets and vad_pump_submit_burst only): RFC 3551 section 4.5.1, 4-bit IMA ADPCM, RTP payload
 * types 5 (8 kHz) and 6 (16 kHz).  A row is the RTP payload as it came off the wire: bytes 0-1 `predict` (int16, big-endian: the
 * decoder's predictor before the first sample), byte 2 `index` (the step index before the first sample; a value above 88 is used as
 * 88), byte 3 reserved (ignored), then the 4-bit codes, two a byte, the first sample in the high nibble.  len_of_row[i] stays the
 * row's length in SAMPLES and must be even; the row takes 4 + len / 2 bytes -- 84 bytes for 20 ms at 8 kHz against 160 of G.711 and
 * 320 of int16.  Every packet carries its own decoder state, so the pump keeps nothing per stream for this format; the device decodes
 * the row (the values of vad_adpcm_expand) on its way into the stream's chunk, and the carry, the tape and a snapshot hold expanded
 * int16 as for every other format.  Results are bit for bit those of the same route fed vad_adpcm_expand of each payload as an S16
 * row.  The corpus routes (vad_upload_rows_coded, _channels), vad_g711_expand and vad_deinterleave go on refusing it.
 * A pump takes DVI4 rows once vad_pump_set_adpcm(p, 1) has enabled them (only while no tick is in flight: VAD_ERR_ARG otherwise;
 * vad_pump_set_adpcm(p, 0) switches them off again; nothing is allocated either way).  A pump on which it was never called refuses
 * codec 3 as a bad codec, as it always did, and runs every route through the code it always ran.                                  */
int  vad_pump_set_adpcm(vad_pump *p, int on);
/* A packet tick whose rows may be G.711: row i of slot r's sample area (seen as streams * N * 2 BYTES) holds len_of_row[i] samples
 * (1 ... N) of stream stream_of_row[i] in format codec_of_row[i] (VAD_PCM_*; NULL = every row VAD_PCM_S16), starting at BYTE offset
 * byte_off_of_row[i], a multiple of 16; the row takes len bytes (G.711) or 2 * len bytes (S16).  The device expands G.711 to int16
 * (the values of vad_g711_expand) on its way into the stream's chunk, so results are bit for bit those of vad_pump_submit_packets fed
 * the expanded int16 packets, and a stream may change its format from one packet to the next.  The payload of an RTP packet goes into
 * the slot as it came off the wire: half the host and link bytes of int16.  Invalid input is VAD_ERR_ARG and nothing is queued: a
 * bad codec, a stream out of range or listed twice, a length out of 1 ... N, a byte offset that is not a multiple of 16 or a row that
 * runs past the slot.  Pending samples, open / close and the chunk routes' refusal behave as for vad_pump_submit_packets.
 * A row with byte_off_of_row[i] == VAD_ROW_SILENT is a silent row of 1 ... N samples (see vad_pump_submit_packets): int16 zeros,
 * also in a G.711 tick (A-law has no code for 0).  Its codec_of_row entry is not looked at -- any byte value is accepted -- and it
 * does not make the tick a G.711 tick.
 * A VAD_PCM_DVI4 row (above; on a pump with vad_pump_set_adpcm) has an even length of 2 ... N samples and takes 4 + len / 2 bytes at its offset: an odd length, a row
 * whose 4 + len / 2 bytes run past the slot and a codec above VAD_PCM_DVI4 are VAD_ERR_ARG like the rest.  A tick with such a row
 * takes a kernel of its own; every other tick runs the code it ran before.                                                         */
int  vad_pump_submit_coded_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row,
                                   const int32_t *len_of_row, const uint8_t *codec_of_row, long n_rows);
/* BURST ticks -- a 60 ms Opus frame is longer than a chunk, a jitter buffer that waited out a stall releases several packets of one
 * stream at once, a stream that fell behind must catch up: in a burst tick a stream may be listed in any number of rows, a row may be
 * longer than N, and a stream that thereby completes several chunks is stepped that many times, in order, inside the one tick.
 * vad_pump_set_burst(p, max_chunks) enables them: 1 ... VAD_PUMP_MAX_BURST chunks per stream and tick (8 chunks are 256 ms: deeper than
 * the jitter buffers this is meant for); only while no tick is in flight (VAD_ERR_ARG otherwise).  It allocates what sub-steps
 * 1 ... max_chunks - 1 need, linear in max_chunks: one device buffer [max_chunks - 1][streams][N] int16 (59 MB at 8 192 streams, 16 kHz,
 * 8 chunks), their flag rows, and page-locked probabilities [ring_slots][max_chunks - 1][streams].  A pump on which it was never called
 * allocates none of that and runs every other route through the code it always ran.
 * vad_pump_submit_burst: rows as in vad_pump_submit_coded_packets (byte offsets, multiples of 16; codec per row or NULL = all S16),
 * except that a stream may be listed more than once and len may exceed N.  Per stream, the samples of its rows are appended, in row
 * order, behind what it has pending; with c pending before and L new samples it completes k = (c + L) / N chunks and keeps
 * (c + L) % N pending.  The tick runs steps = max(1, largest k) sub-steps; sub-step j is a masked step (vad_step_present) of the
 * streams with k > j on their chunk j.  Probabilities, (h, c), context, pending samples and events are bit for bit those of the same
 * pump fed the same concatenated audio, cut into chunks, through vad_pump_submit_rows, one chunk per stream and tick; a burst tick in
 * which no stream is listed twice and no row is longer than N gives exactly what vad_pump_submit_coded_packets gives.  Refused with
 * VAD_ERR_ARG, nothing queued, the pending counts untouched: bursts not enabled; a stream that would complete more than max_chunks
 * chunks; n_rows above `streams` (the row table stays 16 bytes x streams); a bad codec, a stream out of range, len < 1, a misaligned
 * offset, a row that runs past the slot's sample area.  That area stays streams * N * 2 bytes, so not every stream can burst fully in
 * the same tick: the rows of one tick hold at most `streams` chunks of int16 (twice that of G.711).  One H2D copy per tick, as before.
 * vad_pump_poll returns such a tick's events sub-step by sub-step (sub-step 0's in stream order, then sub-step 1's, ...): up to
 * steps x streams of them, and one stream may have a start and an end in the same poll.  vad_pump_burst_steps: the sub-steps slot r's
 * last tick ran (1 for every tick of another route; < 0: bad argument).  vad_pump_burst_probs(p, r, j): [streams] of sub-step j
 * (j = 0: vad_pump_probs(p, r)), VAD_PROB_ABSENT where k <= j; NULL on a bad argument (j beyond max_chunks - 1 included).
 * vad_pump_pending, vad_pump_open / _close and the chunk routes' refusal behave as for packet ticks.
 * A row with byte_off_of_row[i] == VAD_ROW_SILENT is a silent row (see vad_pump_submit_packets) of any length >= 1, longer than N
 * included (after a stall the whole gap may arrive as one row), subject to the max_chunks rule like any row; its codec_of_row entry
 * is not looked at.
 * A VAD_PCM_DVI4 row of a burst (on a pump with vad_pump_set_adpcm) has any even length >= 2 and takes 4 + len / 2 bytes; a row longer than N is decoded in pieces of N
 * samples, the decoder's state carried from piece to piece on the device.                                                          */
#define VAD_PUMP_MAX_BURST 8
int  vad_pump_set_burst(vad_pump *p, int max_chunks);
int  vad_pump_submit_burst(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row, const int32_t *len_of_row,
                           const uint8_t *codec_of_row, long n_rows);
int  vad_pump_burst_steps(const vad_pump *p, int r);
const float *vad_pump_burst_probs(const vad_pump *p, int r, int j);
/* WIDE packet ticks -- WebRTC and Opus decoders deliver 32 / 48 kHz PCM, and the rest of the library takes any multiple of 16 kHz by the
 * reference's rule x[::sr / 16000] (src/silero_vad/utils_vad.py:39-42, :301-304).  A wide tick's rows are int16 samples at step x 16 kHz,
 * and the device keeps every step-th of them on their way into the stream's chunk: no host pass, no per-stream comb bookkeeping in the
 * caller.
 * vad_pump_set_wideband(p, max_step): max_step = 2 (32 kHz) or 3 (48 kHz); anything else, 1 included, is VAD_ERR_ARG.  Only on a 16 kHz
 * pump (VAD_ERR_SAMPLE_RATE on an 8 kHz one: the reference decimates multiples of 16000 only) and only while no tick is in flight
 * (VAD_ERR_ARG otherwise).  It allocates a second page-locked ring of ring_slots WIDE slots and three device landing buffers, each
 * [row table | flags | streams * N * max_step int16] (75 MB on the device, 101 MB page-locked at 8 192 streams, 4 slots, 48 kHz): every
 * stream can deliver a full 32 ms at max_step in the same tick.  Another max_step reallocates (and zeroes every comb phase); the same
 * one is a no-op.  A pump on which it was never called allocates none of that and runs every other route through the code it always
 * ran.  vad_pump_wide_slot(p, r): wide slot r's sample area, streams * N * max_step * 2 bytes; NULL when wideband is not enabled or r is
 * bad.  Ring slot r and wide slot r are the same tick slot: one tick at a time uses r, through either.
 * vad_pump_submit_wide_packets: row i of wide slot r's sample area holds len_of_row[i] int16 INPUT samples of stream stream_of_row[i],
 * sampled at 16000 * step_of_row[i] Hz, starting at BYTE offset byte_off_of_row[i], a multiple of 16.  step = 1 ... max_step;
 * step_of_row == NULL: every row is at max_step.  A row with step 1 is an ordinary 16 kHz packet, so one tick carries 16, 32 and 48 kHz
 * clients side by side.  Rows are int16 only (G.711 is an 8 kHz format).  1 <= len <= step * N: a stream completes at most one chunk per
 * tick, as in vad_pump_submit_packets (a 60 ms Opus frame at 48 kHz goes in over two ticks; there are no wide bursts).
 * Every stream carries a COMB PHASE: input sample number g of the stream is kept iff g % step == 0, g counted from vad_pump_open (or
 * vad_pump_create), or from the row at which the stream's step last changed.  The phase (g % step of the stream's next input sample) is
 * host bookkeeping like the pending count; after a tick is queued it becomes (phase + len) % step.  A row may keep no sample at all
 * (len = 1 at a phase other than 0): it advances the phase and nothing else.  The kept samples are appended to the stream's pending
 * samples -- the same ones every packet route uses, always decimated int16, so a stream may move between wide, packet, coded and burst
 * ticks from one tick to the next (those routes leave the phase alone).  A stream whose pending samples reach N is stepped once, the rest
 * stays pending, every other stream is absent.  Results are bit for bit those of vad_pump_submit_packets fed the rows decimated on the
 * host (vad_decimate with the carried phase).  vad_iter_event.sample and the iterator's current_sample count 16 kHz samples, whatever
 * rate the rows came in at: the reference's VADIterator refuses other rates (utils_vad.py:492), there is no other convention to follow.
 * The chunk routes' refusal of streams with pending samples stays; vad_pump_open / vad_pump_close drop a stream's pending samples, and
 * vad_pump_open zeroes its phase.  Invalid input is VAD_ERR_ARG, nothing is queued, phases and pending counts are untouched: wideband
 * not enabled, a step of 0 or above max_step, a stream out of range or listed twice, a length out of range, a misaligned offset, a row
 * that runs past the area, n_rows above `streams`.  One H2D copy per tick: row table, flags, rows.
 * A row with byte_off_of_row[i] == VAD_ROW_SILENT is a silent row (see vad_pump_submit_packets) of 1 ... step * N INPUT samples at
 * step_of_row[i], which is validated and used as for any row: the phase advances by len and the stream gains the zeros the comb keeps
 * of them; a silent row that keeps no sample advances only the phase.
 * vad_pump_wide_phase: the stream's phase, 0 ... step - 1; < 0: bad argument (wideband not enabled included).                         */
int  vad_pump_set_wideband(vad_pump *p, int max_step);
uint8_t *vad_pump_wide_slot(vad_pump *p, int r);
int  vad_pump_submit_wide_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row, const int32_t *len_of_row,
                                  const uint8_t *step_of_row, long n_rows);
int  vad_pump_wide_phase(const vad_pump *p, int stream);
/* RESAMPLED packet ticks -- speech-synthesis and realtime voice-agent APIs deliver 24 kHz PCM, desktop and browser capture and Bluetooth
 * 44.1 / 22.05 kHz, some telephony 11.025 kHz, and a 48 kHz caller may want read_audio's low-pass instead of the wide route's comb.  A
 * resampled tick's rows are int16 samples at one of the pump's enabled source rates, and the device runs the STREAMING form of the
 * resampler ("resampling to the net's rate" below: vad_resample_stream_ready has the rule) on their way into the stream's chunk: no host
 * pass, no filter state in the caller, int16 at the source rate on the link.
 * vad_pump_set_resample(p, src_rates, n_rates): 1 ... VAD_PUMP_MAX_RATES distinct rates, each one vad_resample_geometry(rate, the pump's
 * rate, ...) serves (VAD_ERR_SAMPLE_RATE otherwise; also for a pair whose chunk of input does not fit the assembly kernel's LDS -- none of
 * the rates named here); on 8 kHz and 16 kHz pumps; only while no tick is in flight (VAD_ERR_ARG otherwise).  It allocates a third
 * page-locked ring of ring_slots RESAMPLE slots and three device landing buffers, each [row table | flags | streams * A int16], A = the
 * input samples of one chunk at the largest enabled rate, ceil(chunk O / N), rounded up to 8 (1 416 for 44.1 -> 16 kHz): every stream can
 * deliver a full 32 ms in the same tick; ONE fp32 batch [streams][chunk], written and read on the compute stream only; an fp32 carry
 * [streams][chunk]; an int16 history [streams][Hmax rounded up to 8], zeroed; and the pairs' tables through the engine's shared ones
 * (vad_resample_reserve).  At 8 192 streams, 4 slots and 44.1 kHz: 94 MB page-locked, 70 MB + 34 MB + 0.7 MB on the device.  The same
 * rates again are a no-op; another set reallocates, unbinds every stream and zeroes every history.  A pump on which it was never called
 * allocates none of that and runs every other route through the code it always ran.  vad_pump_resample_slot(p, r): resample slot r's
 * sample area, streams * A * 2 bytes; NULL when the route is not enabled or r is bad.  Ring slot r, wide slot r and resample slot r are
 * the same tick slot: one tick at a time uses r, through any of them.
 * vad_pump_submit_resampled_packets: row i of resample slot r's sample area holds len_of_row[i] int16 INPUT samples of stream
 * stream_of_row[i], sampled at src_rates[rate_of_row[i]] Hz (rate_of_row == NULL: every row at src_rates[0]), starting at BYTE offset
 * byte_off_of_row[i], a multiple of 16; one tick carries clients of every enabled rate side by side.  Rows are int16 only.  1 <= len <= A.
 * Every stream carries, as host bookkeeping advanced at submit time like the pending count and the comb phase: the rate it is BOUND to,
 * g = the input samples it has received and m = the outputs it has emitted -- both less the same whole periods (O inputs, N outputs), so
 * neither grows with the stream's age --, and c = its fp32 outputs that wait for their chunk, 0 ... chunk - 1.  On the device it carries
 * the last H input samples (vad_resample_stream_history) and those c outputs.  A row of len samples emits the outputs m ... ready(g + len)
 * - 1 of the stream (possibly none: a first row shorter than the filter's latency; possibly two for one input sample when the pair
 * upsamples); they are appended to the c pending ones, a stream whose pending outputs reach the chunk is stepped once on the first chunk
 * of them, the rest stays pending, every other stream is absent.  A row with c + outputs >= 2 chunks is refused: a stream completes at
 * most one chunk per tick (there are no resampled bursts).  One H2D copy per tick: row table, flags, rows.  The assembly kernel
 * (kernel_present.hip assemble_resampled_packets) runs on the compute stream; the masked step behind it is that of every packet tick,
 * reading the fp32 batch.
 * RESULTS.  Every output carries the bits vad_resample_rows_device gives for the stream's concatenated rows (the same table, fp32 fmaf in
 * tap order, a function of the output index alone), whatever the packetisation; probabilities, events, (h, c) and context are bit for bit
 * those of vad_step_present over the chunks y[k chunk : (k + 1) chunk] of that signal, each at the tick its last sample became ready.
 * Nothing is zero-extended on the right: an emitted output never changes, and the filter's tail (at most latency - 1 input samples'
 * worth of outputs) stays unemitted when the stream is closed, like its pending samples on every route.  vad_iter_event.sample counts
 * samples at the pump's rate, as on the wide route.
 * BINDING.  A stream binds to a rate with its first resampled row after vad_pump_create / vad_pump_open.  While bound, a row at another
 * rate is refused, and so is the stream on every other submit route (chunk, rows, packet, coded, burst and wide ticks), in the way the
 * chunk routes refuse a stream with pending samples; a stream with int16 samples pending from those routes cannot take a resampled row.
 * vad_pump_open unbinds the stream and zeroes its counters on the host and its history on the device, ordered behind the ticks in flight
 * like the state reset; vad_pump_close unbinds in the same way and drops the pending outputs.  vad_pump_pending reports c for a bound
 * stream.  vad_pump_resample_state: *src_rate = the rate the stream is bound to (0: none), *inputs_mod = g as defined above, i.e. the
 * inputs received less O * (outputs emitted / N), *pending = c; any pointer may be NULL; VAD_ERR_ARG for a bad stream or a pump without
 * the route.
 * Invalid input is VAD_ERR_ARG, nothing is queued and no count is touched: the route not enabled, a rate index out of range, a stream out
 * of range or listed twice, len < 1 or above A, a misaligned offset, a row that runs past the area, n_rows above `streams`, the binding
 * rules and the two-chunk rule above.
 * A row with byte_off_of_row[i] == VAD_ROW_SILENT is a silent row (see vad_pump_submit_packets) of 1 ... A INPUT samples at its rate:
 * zeros enter the filter (the outputs are not zeros while the history rings out), no bytes of the slot, no offset checks; bit for bit
 * a payload row of int16 zeros.
 * SNAPSHOTS.  vad_pump_export_streams refuses (VAD_ERR_ARG, with a message) a stream that is bound to a rate: blob version 1 has no room
 * for an fp32 carry and a history.  vad_pump_export_streams_v2 writes blob version 2, which carries them with the rate and the counters,
 * and vad_pump_import_streams binds the slot a bound record enters; a version 1 record, or an unbound one, leaves its slot unbound.     */
#define VAD_PUMP_MAX_RATES 4
int  vad_pump_set_resample(vad_pump *p, const int *src_rates, int n_rates);
uint8_t *vad_pump_resample_slot(vad_pump *p, int r);
int  vad_pump_submit_resampled_packets(vad_pump *p, int r, const int32_t *stream_of_row, const int32_t *byte_off_of_row,
                                       const int32_t *len_of_row, const uint8_t *rate_of_row, long n_rows);
int  vad_pump_resample_state(const vad_pump *p, int stream, int *src_rate, long *inputs_mod, long *pending);
/* The host twin of the device's decimation, from the same definition: the samples of in[0 .. n) that the comb keeps -- in[k] with
 * (phase + k) % step == 0, i.e. in[(-phase) % step :: step] -- are written to out, and their number is returned.  phase = the number of
 * the stream's samples in front of in[0], modulo step; the next piece's phase is (phase + n) % step.  Host only, re-entrant.
 * -VAD_ERR_ARG for step < 1, phase out of 0 ... step - 1, n < 0 or a NULL buffer with n > 0.                                       */
long vad_decimate(int step, int phase, const int16_t *in, long n, int16_t *out);
/* n samples in format `codec` at `in` (n bytes for G.711, n int16 for VAD_PCM_S16: copied) -> out[0 .. n) int16 on the host: ITU-T
 * G.711 expansion, the values of Python's audioop.ulaw2lin / alaw2lin(x, 2), from the same definition the device uses.  VAD_OK, or
 * VAD_ERR_ARG for a bad codec, n < 0 or a NULL buffer with n > 0.                                                               */
int  vad_g711_expand(int codec, const uint8_t *in, long n, int16_t *out);
/* A DVI4 payload (VAD_PCM_DVI4: 4 header bytes, then 4-bit codes) of nbytes bytes at `payload` -> out[0 .. 2 * (nbytes - 4)) int16 on
 * the host, from the same single-code step the device uses: the values of Python's audioop.adpcm2lin(payload[4:], 2, (predict,
 * min(index, 88))).  Returns the samples written; nbytes == 4 (a header alone) gives 0 and looks at neither pointer.  -VAD_ERR_ARG for
 * nbytes < 4 or a NULL pointer with nbytes > 4.  Host only, re-entrant.                                                              */
long vad_adpcm_expand(const uint8_t *payload, long nbytes, int16_t *out);
/* Samples of `stream` submitted in packets and not yet stepped (0 ... N - 1; host bookkeeping, no synchronisation); < 0: bad argument. */
long vad_pump_pending(const vad_pump *p, int stream);
/* Retire the OLDEST submitted tick: wait for it (block != 0) or return VAD_PUMP_BUSY, run the iterator logic of every open
 * stream over its probabilities and write the tick's events (stream order; at most `cap`, the return value is how many there
 * were, <= streams; a burst tick: <= its sub-steps x streams).  *slot = the ring slot that is free again.  The probabilities stay readable in vad_pump_probs(p, slot)
 * until that slot's next tick.                                                                                             */
long vad_pump_poll(vad_pump *p, int block, vad_iter_event *out, long cap, int *slot);
const float *vad_pump_probs(const vad_pump *p, int r);   /* [streams] */
/* A new stream takes slot `stream`: zero (h, c), context and iterator state, ordered behind the ticks already submitted
 * (reset_states, JIT!/vad/model/vad_annotator.py:157-162 + utils_vad.py:500-505).  close: the slot is still computed (lock-step
 * batch) but emits no events.  Both take effect BEHIND the ticks that are in flight when they are called, on the device (stream
 * order) and on the host (the iterator state is reset / muted when those ticks have been retired: their probabilities and events
 * belong to the slot's previous occupant).                                                                                 */
int  vad_pump_open(vad_pump *p, int stream);
int  vad_pump_close(vad_pump *p, int stream);
/* Test / migration hook: copy stream's carried h[128], c[128], ctx[C] to the host (any may be NULL).  Synchronises.        */
int  vad_pump_state(vad_pump *p, int stream, float *h, float *c, float *ctx);

/* THE TAPE: every stream's recent audio kept on the device, fetched by sample range.  The consumer of a VAD front end (an ASR or a
 * diarisation model) wants the utterance behind an END event, at the rate and in the form the net heard it -- the reference's own flow is
 * VADIterator events, then the slice audio[start:end].  On the packet routes the host never has that audio: G.711 rows are expanded on
 * the device, 32 / 48 kHz rows are combed there at a phase only the pump knows, silent rows exist only as zeros spliced in there.  With a
 * tape the pump keeps, per stream, a ring of the last `chunks` chunks it stepped the stream on -- written on the device as a side effect
 * of every step of every route (full, masked, compact, rows, packets, coded, burst, wide), from the very rows the step kernels read --
 * and copies any still-held sample range of any set of streams out, packed.
 *
 * THE CLOCK.  Two int64 counters per stream live on the device: `count`, the chunks stepped since the stream's clock started, and
 * `floor`, the first chunk the tape can hold.  A stream that is stepped (its flag is set, or the tick has no flags) has its chunk taped
 * into ring slot count % chunks and its count incremented; a stream that is absent from a step is untouched.  vad_pump_open zeroes both
 * counters in compute-stream order, behind the ticks in flight, exactly as it zeroes (h, c): so for every open stream count * N is
 * the iterator's current_sample at every tick boundary, and the sample numbers of the events ARE tape positions.  vad_pump_close
 * changes nothing (a closed stream that a full tick still steps is taped; the next open restarts its clock).  vad_pump_import_streams
 * into a pump with a tape sets count = current_sample / N of the record: the clock continues; a version 1 or 2 record sets floor = count,
 * nothing before the import is held, a version 3 record that carries a run of the source's tape sets floor = count - the chunks kept.
 * Snapshot blobs of versions 1 and 2 do not carry the tape: they are unchanged, and a pump with a tape exports the bytes one without it
 * does.  Blob version 3 (SNAPSHOT AND RESTORE below) carries, per stream, the newest whole chunks from a sample position the caller names.
 *
 * THE WINDOW.  With held_lo = max(floor, count - chunks) * N and held_hi = count * N the tape holds the samples [held_lo, held_hi) of
 * the stream's clock.  A request [start, end), start <= end, of ANY int64 values is confined to it:
 *     first = min(max(start, held_lo), held_hi),  last = min(max(end, first), held_hi),  n = last - first
 * (csrc/tape.hpp, the one source of the rule).  first > start: the head of the range is no longer held (or lies before the clock).
 * vad_tape_window: the rule for given counters -> *first, *n.  Host only, re-entrant, no GPU.  VAD_ERR_ARG: start > end, chunks < 2,
 * N < 1, count < 0, or counters whose product with N is no int64.
 * THE RUN a version 3 snapshot carries for a stream is whole chunks, from the chunk that holds sample `from` to the newest one, as far as
 * the tape holds them: with held_lo = max(floor, count - chunks), in CHUNKS,
 *     first_chunk = min(max(from / N, held_lo), count),  n_chunks = count - first_chunk
 * where `from` is clamped into [held_lo * N, count * N] before it is divided: any int64 is legal (a negative value or one before the
 * window gives everything held, one at or behind count * N gives nothing), and a position in the middle of a chunk rounds down to its
 * chunk.  vad_tape_run: that rule for given counters -> *first_chunk, *n_chunks.  Host only, re-entrant, no GPU.  VAD_ERR_ARG: chunks < 2,
 * N < 1, count < 0, floor < 0, or counters whose product with N is no int64.
 *
 * vad_pump_set_tape: once, before the pump's first tick, chunks >= 2 (any value, not only powers of two).  Allocates
 * [streams][chunks][N] int16 and the counters, all zero.  VAD_ERR_ARG with nothing changed: after a tick was submitted, a second call,
 * chunks < 2, a pump with vad_pump_set_resample enabled -- and vad_pump_set_resample on a pump with this tape: that route steps an fp32
 * batch, an int16 tape of it would not be what the net saw (THE FP32 TAPE below holds it).  VAD_ERR_ALLOC: no device memory; the pump stays usable without a tape.  A
 * pump that never calls it allocates nothing and launches nothing for it.
 * SIZING.  streams x chunks x N x 2 bytes: 8192 streams x 512 chunks (16.4 s) = 4.3 GB.  A sample stays fetchable for `chunks` chunks of
 * ITS stream, counted from when it is stepped -- ticks in flight count: up to ring_slots x max_chunks chunks.  Size chunks as the
 * longest utterance + speech_pad + that slack.
 *
 * FETCHING, both from the thread that drives the pump.
 * vad_pump_tape_window: synchronises the compute stream -- so it sees every tick submitted so far, retired or in flight -- reads the
 * counters and applies the rule to request i = (stream[i], [start[i], end[i])) -> first[i], count[i]; returns the total number of
 * samples (>= 0).  A stream may appear in any number of requests; n == 0 is fine.  -VAD_ERR_ARG with nothing written: a pump without a
 * tape, a stream out of range, start > end.
 * vad_pump_fetch_audio: request i's count[i] samples from sample first[i] of stream[i]'s clock go to out + out_offset[i] (in samples).
 * An exclusive sum of the counts, each rounded up to 8, keeps every start 16-byte aligned (the gather kernel's fast path); any other
 * offset is honoured element by element.  EXACTLY count[i] samples are written per request: what lies between the requests and behind
 * the last one is not touched.  out_on_device == 0: `out` is host memory -- the samples are packed in a device buffer that grows on
 * demand, cross the link in ONE copy and are dealt out on the host; out_on_device == 1: `out` is device memory of the pump's GPU, for a
 * consumer there, and the kernel writes it directly.  Synchronous: the samples are in `out` on return.  The call synchronises first and
 * checks every range again, by the same rule, against the counters as they are then: a range with count[i] > 0 that is not wholly
 * inside its stream's window is VAD_ERR_ARG, "no longer held", and nothing is written (a tick submitted between the two calls taped
 * over it).  Also VAD_ERR_ARG: a pump without a tape, a stream out of range, a negative count or offset.  It touches none of the
 * pump's carried state and works with ticks in flight.
 * vad_pump_tape_state: test hook -> *count, *floor of one stream (either may be NULL).  Synchronises.
 *
 * THE FP32 TAPE.  vad_pump_set_tape_f32 makes the tape's element what the net read: float32.  It allocates [streams][chunks][N] float and
 * the same two counters a stream, by the rules of vad_pump_set_tape (once, before the first tick, chunks >= 2 of any value, VAD_ERR_ALLOC
 * leaves the pump usable without a tape).  A pump holds at most ONE tape: either set call on a pump that has either tape is VAD_ERR_ARG
 * ("already").  Unlike the int16 tape it goes together with vad_pump_set_resample, in either order -- a pump of 44.1 / 24 / 22.05 /
 * 11.025 kHz clients is the one whose net-rate audio the host never holds.  What it tapes is every step of every route: a resampled tick
 * tapes its rows of the fp32 batch bit for bit (the values vad_resample_rows_device gives for the stream's concatenated rows); a step
 * over int16 rows (full, masked, compact, rows, packets, coded, burst sub-steps, wide) tapes (float)x * (1.0f / 32768.0f), the value the
 * frontend computes from that sample, exact, in [-1, 1).  Bound and unbound streams of one pump share the one tape.  A second
 * vad_pump_set_resample with other rates unbinds every stream, as ever, and leaves the tape and its clocks alone.  The clock, the window
 * rule, vad_pump_open / close / import_streams, the exports (versions 1 and 2 do not carry it, version 3 carries its floats as they are) and vad_tape_window / vad_pump_tape_window /
 * vad_pump_tape_state are those of the int16 tape: none of them depends on the element.
 * SIZING.  streams x chunks x N x 4 bytes: 8192 streams x 512 chunks = 8.6 GB.
 * vad_pump_fetch_audio_f32: the contract of vad_pump_fetch_audio with "sample" meaning one float -- it synchronises, re-checks every
 * range ("no longer held", nothing written), writes EXACTLY count[i] floats per request to out + out_offset[i] (in floats), stages a host
 * destination through one D2H copy and lets the kernel write a device destination.  An exclusive sum of the counts, each rounded up to 4
 * (or 8), keeps every start 16-byte aligned for the gather kernel's vector path; any other offset is honoured float by float.
 * THE WRONG FETCH for the pump's tape -- vad_pump_fetch_audio on an fp32 tape, vad_pump_fetch_audio_f32 on an int16 tape -- is
 * VAD_ERR_ARG with a message that names the right call; nothing is written and the pump stays usable.
 * vad_pump_tape_format: 0 = no tape, 2 = the int16 tape, 4 = the fp32 tape (the element's size in bytes); -VAD_ERR_ARG for NULL.  Host
 * only, no synchronisation.                                                                                                          */
int  vad_tape_window(int64_t count, int64_t floor, int chunks, int N, int64_t start, int64_t end, int64_t *first, int64_t *n);
int  vad_tape_run(int64_t count, int64_t floor, int chunks, int N, int64_t from, int64_t *first_chunk, int64_t *n_chunks);
int  vad_pump_set_tape(vad_pump *p, int chunks);
long vad_pump_tape_window(vad_pump *p, const int32_t *stream, const int64_t *start, const int64_t *end, long n, int64_t *first, int64_t *count);
int  vad_pump_fetch_audio(vad_pump *p, const int32_t *stream, const int64_t *first, const int64_t *count, long n, const int64_t *out_offset,
                          int16_t *out, int out_on_device);
int  vad_pump_tape_state(vad_pump *p, int stream, int64_t *count, int64_t *floor);
int  vad_pump_set_tape_f32(vad_pump *p, int chunks);
int  vad_pump_fetch_audio_f32(vad_pump *p, const int32_t *stream, const int64_t *first, const int64_t *count, long n, const int64_t *out_offset,
                              float *out, int out_on_device);
int  vad_pump_tape_format(const vad_pump *p);

/* SNAPSHOT AND RESTORE of live streams: everything a stream carries from one tick to the next leaves a pump as plain bytes and enters
 * any slot of any pump of the same sample rate -- another GPU, another process, another machine -- for a drain, a rebalancing of
 * streams between per-GPU ranks, a rolling restart or a failover.  The reference treats this state as the resumable unit of the model
 * (_state and _context are explicit inputs and outputs of its graph; the VADIterator adds triggered / temp_end / current_sample,
 * utils_vad.py:500-503).  Every probability, event, state and pending count after an import is bit for bit what the uninterrupted
 * stream would have produced, PROVIDED the destination pump was created with the iterator parameters of the source (see below).
 *
 * THE BLOB (version 1).  Little-endian; this layout is the contract between a blob's writer and its readers.
 *   header, VAD_SNAPSHOT_HEADER_BYTES = 64:
 *      0  char    magic[8]       "SVADSNAP"
 *      8  uint32  version        VAD_SNAPSHOT_VERSION
 *     12  uint32  header_bytes   64
 *     16  int32   sr             8000 / 16000
 *     20  int32   N              samples per chunk at sr (256 / 512)
 *     24  int32   C              context samples at sr (32 / 64)
 *     28  uint32  stride         bytes per record: 32 + 4 * (128 + 128 + C) + 2 * N = 1696 / 2336, a multiple of 16
 *     32  int64   n_records
 *     40  float64 threshold      \  the source pump's iterator parameters as the iterator compares them: the threshold, and
 *     48  float64 min_silence     > min_silence_duration_ms and speech_pad_ms in SAMPLES at sr.  INFORMATIONAL: import does not compare
 *     56  float64 pad            /  them with the destination's, and the continuation is bit-identical only if they are the same.
 *   then n_records records of `stride` bytes, each:
 *      0  vad_stream_info (32 bytes, below)
 *     32  float32 h[128]
 *    544  float32 c[128]
 *   1056  float32 ctx[C]                  the context the stream's NEXT chunk is computed behind
 *   1056 + 4 C  int16 pending_samples[N]  the stream's samples that wait for their chunk (at the pump's rate: G.711 rows expanded,
 *                                         wide rows decimated), pending_samples[0 : pending]; everything behind them is ZERO
 * A record does not name the slot it came from.  Reserved bytes are written as zero and a reader refuses a record in which they are not;
 * samples behind `pending` are written as zero and ignored when read.  Two exports with no tick between them are byte for byte the same.
 * NOT carried: ticks in flight (there are none: see below), the position counter of the vad_pump_play* helpers (it restarts as after
 * vad_pump_open), burst / wideband being enabled (properties of a pump, not of a stream), in versions 1 and 2 the tape (THE TAPE above: a
 * pump with a tape writes the same bytes, and an import of such a record restarts the slot's tape at the record's current_sample;
 * version 3 below carries it), and the model weights.
 *
 * THE BLOB (version 2) carries, in addition, what a stream that is BOUND to a resampled rate holds (vad_pump_submit_resampled_packets):
 * its rate, its two counters, its fp32 pending outputs and its filter history.  vad_pump_export_streams_v2 writes it, for bound and
 * unbound streams alike; vad_pump_export_streams goes on writing version 1.
 *   header, VAD_SNAPSHOT_HEADER_BYTES_V2 = 96:
 *      0  the 64 bytes of the version 1 header, with version = VAD_SNAPSHOT_VERSION_2, header_bytes = 96 and
 *         stride = the version 1 stride + 32 + 4 * N + 2 * 160 = 3072 / 4736, a multiple of 16
 *     64  uint8   reserved[32]   zero
 *   then n_records records of `stride` bytes, each:
 *      0  the version 1 record, unchanged (S1 = the version 1 stride, 1696 / 2336 bytes)
 *     S1  vad_resample_info (32 bytes, below)
 *     S1 + 32        float32 carry[N]       the outputs that wait for their chunk, carry[0 : pending_out]; everything behind them is +0.0f
 *     S1 + 32 + 4 N  int16   history[160]   the last H = vad_resample_stream_history(src_rate, sr) INPUT samples at src_rate, oldest
 *                                           first, zeros where the stream has not lived that long: history[0 : H]; everything behind
 *                                           them is ZERO.  VAD_SNAPSHOT_HISTORY = 160 holds every served pair's H (K <= 160 in
 *                                           vad_resample_geometry, H = K - 1) and does not depend on the rates either pump enabled.
 * src_rate is in Hz, never a rate index: the destination may have enabled its rates in another order.  A record of a stream that is
 * bound to no rate has src_rate = 0 and an all-zero tail behind its version 1 part, and that part is byte for byte the version 1 record.
 * The fields of a record with src_rate != 0, as the submit path produces them and as every reader demands them (O, N_r = the pair's O and
 * N of vad_resample_geometry(src_rate, sr), ready = vad_resample_stream_ready(src_rate, sr, .)):
 *   src_rate     a pair (src_rate, sr) with a streaming form: vad_resample_stream_history(src_rate, sr) >= 0
 *   pending_out  0 ... N - 1 (N = the chunk)
 *   outputs_mod  0 ... N_r - 1: the outputs emitted, less whole periods
 *   inputs_mod   >= 0 with ready(inputs_mod) == outputs_mod -- the inputs received less O per dropped period; since ready(g) >= N_r from
 *                the g on at which period 0 is complete, this also bounds it: inputs_mod < the smallest g with ready(g) == N_r (<= the
 *                latency + O)
 *   vad_stream_info.pending == 0: a bound stream has no int16 samples pending (BINDING above)
 *   reserved bytes zero; carry[pending_out : N] all bits zero; history[H : 160] zero
 * and with src_rate == 0 every other byte of the tail is zero.  A version 1 layout that merely says version 2 is refused: header_bytes
 * and stride differ.
 *
 * THE BLOB (version 3) carries, in addition, a RUN of each stream's tape (THE TAPE above): the newest whole chunks of the audio the net
 * heard, from a sample position the caller names per stream -- typically the START of the utterance the stream is in, so that the END
 * event on the destination finds its audio there.  vad_pump_export_streams_v3 writes it; the other two exports write what they wrote.
 *   header, VAD_SNAPSHOT_HEADER_BYTES_V3 = 128:
 *      0  the 64 bytes of the version 1 header, with version = VAD_SNAPSHOT_VERSION_3, header_bytes = 128 and
 *         stride = the version 2 stride + 32 = 3104 / 4768, a multiple of 16
 *     64  int32   tape_elem      the element of the source's tape in bytes, vad_pump_tape_format: 0 (no tape), 2 (int16), 4 (float32)
 *     68  int32   reserved       zero
 *     72  int64   tape_bytes     the bytes of the tape section
 *     80  uint8   reserved[48]   zero
 *   then n_records records of `stride` bytes, each:
 *      0  the version 2 record, unchanged, byte for byte (S2 = the version 2 stride, 3072 / 4736 bytes)
 *     S2  vad_tape_info (32 bytes, below)
 *   then the TAPE SECTION, tape_bytes bytes from byte 128 + n_records * stride on: the runs of the records in record order, without
 *   gaps or padding.  Record i's run is n_chunks * N * tape_elem bytes at `offset` from the section's start: the chunks first_chunk ...
 *   first_chunk + n_chunks - 1 of the stream's clock, oldest first, each N elements of tape_elem bytes as the tape held them.  The blob is
 *   EXACTLY 128 + n_records * stride + tape_bytes bytes (a version 3 blob in a longer or a shorter buffer is refused).
 * The writer carries a run only for a stream whose tape clock is its iterator clock, count * N == current_sample -- every open stream
 * (THE CLOCK above); any other stream, every stream of a pump without a tape, and a stream whose run is empty has an ALL-ZERO
 * vad_tape_info.  The fields, as the writer produces them and as every reader demands them:
 *   tape_elem 0, 2 or 4; tape_bytes >= 0; with tape_elem == 0: tape_bytes == 0 and every vad_tape_info all zero
 *   first_chunk >= 0; 0 <= n_chunks <= tape_bytes / (N * tape_elem) less the chunks of the earlier runs (checked before anything is
 *   multiplied); reserved bytes zero
 *   n_chunks == 0: first_chunk == 0 and offset == 0
 *   n_chunks > 0:  offset == the bytes of all earlier runs, and (first_chunk + n_chunks) * N == current_sample of the record
 *   the bytes of all runs == tape_bytes, and the buffer holds exactly header + records + tape_bytes
 * The audio itself is payload, like h and c.  The version 2 part of every record is held to the version 2 rules.  A version 2 layout
 * that merely says version 3 is refused: header_bytes and stride differ.  Two exports with no tick between them are byte for byte the
 * same.                                                                                                                             */
#define VAD_SNAPSHOT_VERSION 1
#define VAD_SNAPSHOT_HEADER_BYTES 64
#define VAD_SNAPSHOT_VERSION_2 2
#define VAD_SNAPSHOT_HEADER_BYTES_V2 96
#define VAD_SNAPSHOT_VERSION_3 3
#define VAD_SNAPSHOT_HEADER_BYTES_V3 128
#define VAD_SNAPSHOT_HISTORY 160
typedef struct vad_stream_info {
    int64_t current_sample;      /* VADIterator.current_sample: samples stepped since vad_pump_open; >= 0                            */
    int64_t temp_end;            /* VADIterator.temp_end: 0 ... current_sample                                                       */
    int32_t pending;             /* samples that wait for their chunk, 0 ... N - 1 (vad_pump_pending)                                */
    uint8_t active;              /* 1: open (emits events); 0: closed (vad_pump_close)                                               */
    uint8_t triggered;           /* VADIterator.triggered, 0 / 1: inside a speech segment                                            */
    uint8_t wide_step;           /* the step of the stream's last wide row: 0 = it never had one, else 1 ... 3                       */
    uint8_t wide_phase;          /* its comb phase (vad_pump_wide_phase), 0 ... max(1, wide_step) - 1                                */
    uint8_t reserved[8];         /* zero                                                                                             */
} vad_stream_info;
typedef struct vad_resample_info {   /* the host's part of a version 2 record's tail; the ranges are stated above                        */
    int32_t src_rate;            /* the rate the stream is bound to, in Hz; 0: none, and everything below is zero                    */
    int32_t pending_out;         /* c: fp32 outputs that wait for their chunk (vad_pump_pending of a bound stream)                   */
    int64_t inputs_mod;          /* g: input samples received, less whole periods (vad_pump_resample_state)                          */
    int64_t outputs_mod;         /* m: outputs emitted, less the same whole periods                                                  */
    uint8_t reserved[8];         /* zero                                                                                             */
} vad_resample_info;
typedef struct vad_tape_info {       /* behind a version 3 record's version 2 part: its run in the tape section; the rules are stated above */
    int64_t first_chunk;         /* the run's first chunk, a chunk number of the stream's clock; 0 with an empty run                 */
    int64_t n_chunks;            /* whole chunks of N elements; (first_chunk + n_chunks) * N == current_sample where > 0             */
    int64_t offset;              /* of the run in the tape section, in bytes; 0 with an empty run                                    */
    uint8_t reserved[8];         /* zero                                                                                             */
} vad_tape_info;
/* Bytes of a blob of n records at sample rate sr: 64 + n * stride.  0 for a bad sr or n < 0.  Host only.  _v2: 96 + n * the version 2
 * stride.                                                                                                                           */
size_t vad_pump_snapshot_bytes(int sr, long n);
size_t vad_pump_snapshot_bytes_v2(int sr, long n);
/* Bytes of a version 3 blob of n records of a tape of tape_elem-byte elements whose runs have total_chunks chunks together: 128 + n *
 * the version 3 stride + total_chunks * N * tape_elem.  0 for a bad sr, n < 0, tape_elem other than 0 / 2 / 4, total_chunks < 0 (or
 * > 0 with tape_elem == 0) or a size that is no size_t.  Host only.                                                                  */
size_t vad_snapshot_bytes_v3(int sr, long n, int tape_elem, int64_t total_chunks);
/* EXPORT: the records of streams[0 ... n - 1] (distinct slots; NULL = every slot in ascending order, and n must be the pump's stream
 * count) into blob[0 : vad_pump_snapshot_bytes(sr, n)], ordinary host memory of `cap` bytes.  Read-only: the pump and the exported
 * streams go on exactly as if the call had not happened; the caller closes them when it wants to.  Synchronous: the blob is complete on
 * return.  One gather kernel on the pump's compute stream packs the records on the device and ONE copy brings them over the link.
 * IMPORT: record records[i] of the blob (NULL = record i) replaces the whole carried state of slot streams[i], i = 0 ... n - 1
 * (distinct slots; records may repeat and may be any subset, so one blob can be dealt out to several pumps): h, c, the context the next
 * tick reads, the pending samples and their count, the comb step and phase, the iterator state and the open / closed flag; the
 * position counter of vad_pump_play* restarts.  Synchronous.  ONE copy takes the records blob[min record ... max record] over the link
 * and one scatter kernel on the compute stream puts them in place.
 * BOTH work only on an IDLE pump -- no tick in flight (retire them with vad_pump_poll first: at most ring_slots - 1), VAD_ERR_ARG
 * otherwise, as vad_pump_set_burst / vad_pump_set_wideband: then no deferred open / close is waiting and the host bookkeeping, which
 * advances partly at submit time (pending counts, comb phases) and partly at retire time (iterator state), is at ONE point of every
 * stream's timeline.  A poisoned pump refuses them like every other call (VAD_ERR_HIP).
 * Export refuses (VAD_ERR_ARG, blob untouched): a slot out of range or listed twice, n < 0, cap too small.
 * Import refuses, with NOTHING queued and NOTHING changed: a blob vad_snapshot_inspect refuses (VAD_ERR_ARG: bad magic / version /
 * geometry, shorter than its header claims, any record field out of its range -- a blob is untrusted input, and all of it is checked on
 * the host before a value from it can steer a device address or a loop bound); a sample rate other than the pump's
 * (VAD_ERR_SAMPLE_RATE); a record index out of range, a slot out of range or listed twice, a record with wide_step >= 2 for a pump
 * whose wideband max_step is smaller (a pump without wideband included) (VAD_ERR_ARG).  A record with wide_step 1 enters a pump
 * without wideband as a stream that never had a wide row: a step-1 comb has no phase to lose.
 * RESAMPLED STREAMS.  vad_pump_export_streams writes version 1 and refuses a stream that is bound to a rate (VAD_ERR_ARG).
 * vad_pump_export_streams_v2: the same call with the same rules -- idle pump, read-only, synchronous, one gather kernel, one copy -- into
 * blob[0 : vad_pump_snapshot_bytes_v2(sr, n)], version 2, bound and unbound streams alike, on a pump with or without the resampled route.
 * vad_pump_import_streams takes both versions.  A version 1 record, and a version 2 record with src_rate == 0, leave the slot bound to
 * no rate (a slot that was bound is unbound and its history zeroed, as by vad_pump_open).  A version 2 record with src_rate != 0
 * replaces, besides everything above, the slot's whole resampled state: the binding (to the index src_rate has among the DESTINATION's
 * rates) and the counters g, m, c on the host; the whole fp32 carry row and the whole history row, at the destination's own pitch, on the
 * device -- zeros behind c and behind H whatever the blob and the slot held before.  Refused in addition, with nothing queued and
 * nothing changed (VAD_ERR_ARG): a record whose src_rate is not among the destination's enabled rates (a pump without the route
 * included), and -- already by vad_snapshot_inspect -- any field outside the ranges stated with the layout.
 * THE TAPE IN A SNAPSHOT.  vad_pump_export_streams_v3: the version 2 export with the same rules -- idle pump, read-only, synchronous, the
 * same refusals, the records by the same gather kernel and copy -- into a version 3 blob.  tape_from[i] is the sample position of
 * streams[i]'s clock from which its audio is wanted (any int64; NULL: everything each stream's tape holds); the run is THE RUN of
 * (count, floor, tape_from[i]) as the counters are then, for a stream with count * N == current_sample, and empty for any other.  A
 * second kernel on the compute stream packs the runs on the device, in record order, and ONE more copy brings them over.  On a pump
 * without a tape tape_from is ignored and the blob has tape_elem = 0 and no tape section.  `cap` must hold what
 * vad_pump_snapshot_plan_v3 says: that call synchronises the compute stream, reads the counters, applies the same rule to the same
 * arguments and returns the bytes of the blob the export would write (0, with a message: a NULL pump, a bad slot list).  It changes
 * nothing and works with ticks in flight, but only between an idle pump's plan and its export is the figure certain to be the same.
 * The staging of the runs, device memory, is allocated by the first export that carries one and grows on demand; a pump that never
 * makes these calls allocates nothing for them, and no tick does anything for them.
 * vad_pump_import_streams takes version 3 as well.  Everything a version 2 record replaces, it replaces as before.  Into a pump whose
 * tape has the blob's element, a record with n_chunks > 0 brings its audio along: kept = min(n_chunks, the destination's chunks), the
 * newest `kept` chunks of the run land in ring slots c % chunks of the DESTINATION's ring (whatever the source's ring length was and
 * whatever the slot's ring held), count = current_sample / N as ever and floor = count - kept -- so vad_pump_fetch_audio on the
 * destination returns the stream's audio across the migration point.  A record with an empty run, and every record of versions 1 and
 * 2, leaves count = floor.  A destination without a tape ignores the tape section; a blob with tape_elem == 0 enters a taped pump like a
 * version 2 blob.  A blob whose tape_elem and the pump's are both non-zero and DIFFER (an int16 run for an fp32 tape, or the reverse) is
 * refused with VAD_ERR_ARG, nothing queued and nothing changed: the import does not convert.  The tape bytes of the selected records
 * cross the link in ONE copy, the span from the first selected run to the last, and one scatter kernel puts them in place.           */
int  vad_pump_export_streams(vad_pump *p, const int32_t *streams, long n, void *blob, size_t cap);
int  vad_pump_export_streams_v2(vad_pump *p, const int32_t *streams, long n, void *blob, size_t cap);
size_t vad_pump_snapshot_plan_v3(vad_pump *p, const int32_t *streams, long n, const int64_t *tape_from);
int  vad_pump_export_streams_v3(vad_pump *p, const int32_t *streams, long n, const int64_t *tape_from, void *blob, size_t cap);
int  vad_pump_import_streams(vad_pump *p, const void *blob, size_t nbytes, const int32_t *records, const int32_t *streams, long n);
/* Readers of a blob of any version; host only, no pump and no device needed.  vad_snapshot_inspect: validate ALL of blob[0 : nbytes]
 * (header and every record's fields; versions 2 and 3: also every byte that has to be zero; version 3: every vad_tape_info, the sums and
 * the buffer's exact size) -> VAD_OK and *n_records, *sr (either may be
 * NULL), or VAD_ERR_ARG.  vad_snapshot_stream: the version 1 part of record i of a valid blob -> *info, h[128], c[128], ctx[C],
 * pending[N] (any may be NULL); VAD_ERR_ARG for an invalid blob or i out of range.  vad_snapshot_resample: the tail of record i ->
 * *info, carry[N], history[VAD_SNAPSHOT_HISTORY] (any may be NULL); a version 1 blob has no tail: all three come back zero.
 * vad_snapshot_tape: the run of record i -> *info and, with audio != NULL, its n_chunks * N * tape_elem bytes to audio[0 : cap]
 * (VAD_ERR_ARG with nothing written if cap, in bytes, is smaller; the element is tape_elem at byte 64 of the header).  A blob of
 * version 1 or 2 has no runs: *info comes back zero and nothing is written to audio.                                                 */
int  vad_snapshot_inspect(const void *blob, size_t nbytes, long *n_records, int *sr);
int  vad_snapshot_stream(const void *blob, size_t nbytes, long i, vad_stream_info *info, float *h, float *c, float *ctx, int16_t *pending);
int  vad_snapshot_resample(const void *blob, size_t nbytes, long i, vad_resample_info *info, float *carry, int16_t *history);
int  vad_snapshot_tape(const void *blob, size_t nbytes, long i, vad_tape_info *info, void *audio, size_t cap);

/* The whole loop in one native call -- for tests, benchmarks and file-fed servers: stream b plays rows[b * ld ...] circularly with
 * period `period` samples (a multiple of N): at tick t its chunk is rows[b * ld + (t * N) % period ...].  `fill_threads` SOURCE
 * threads (0: min(8, vad_host_threads() - 2); < 0: the sources are silent, the slots keep their content -- isolates the device
 * side) each own a range of streams and WRITE their chunks into ring slot t % ring_slots for t = first_tick ... first_tick +
 * n_ticks - 1; the calling thread submits a tick once it is completely written and, once `depth` ticks are in flight (clamped to
 * 1 ... ring_slots - 1), retires the oldest.  depth 1 = strictly one tick at a time (the next chunks are written after the
 * previous tick's events are out): tick_ms_* is then the latency of one tick, slot written -> events on the host; depth >= 2: the
 * sources write the next tick while `depth` ticks are in flight.  All events are appended to `out` (at most
 * cap; the return value is their number) and `st` (may be NULL) is filled in (fill_ms_mean: per source thread and tick).          */
long vad_pump_play(vad_pump *p, const int16_t *rows, long ld, long period, long first_tick, long n_ticks, int depth, int fill_threads,
                   vad_iter_event *out, long cap, vad_pump_stats *st);
/* The same loop with streams that miss ticks: pattern = [pattern_ticks][streams] bytes, stream b has a chunk at tick t iff
 * pattern[(t % pattern_ticks) * streams + b] != 0.  A stream's audio advances only when it delivers (its k-th delivered chunk is
 * rows[b * ld + (k * N) % period ...], k counted since the stream was opened): a late packet delays the stream, it does not skip
 * audio.  The sources write the flags into the slot's flag row and every tick is a vad_pump_submit_present.  pattern == NULL:
 * vad_pump_play.                                                                                                            */
long vad_pump_play_gaps(vad_pump *p, const int16_t *rows, long ld, long period, const uint8_t *pattern, long pattern_ticks, long first_tick,
                        long n_ticks, int depth, int fill_threads, vad_iter_event *out, long cap, vad_pump_stats *st);
/* vad_pump_play_gaps with compact slots: the sources write the delivering streams' chunks back to back (a source thread's first row is
 * the number of delivering streams in front of its range) and every tick is a vad_pump_submit_compact.  Same events, same state.    */
long vad_pump_play_compact(vad_pump *p, const int16_t *rows, long ld, long period, const uint8_t *pattern, long pattern_ticks, long first_tick,
                           long n_ticks, int depth, int fill_threads, vad_iter_event *out, long cap, vad_pump_stats *st);

/* ---- host-side ingest ---------------------------------------------------------------------------------
 * Pack n recordings of different lengths (lens[i] samples of elem_size 2 = int16, 4 = float32 or 1 = G.711 codes, packed as bytes, at
 * rows[i]) into one zero-padded row-major [n][width] batch at dst (typically pinned host memory that
 * is then copied to the GPU and handed to vad_forward_audio[_i16]).  Zero padding on the right is what
 * the reference does to a recording's last chunk (src/silero_vad/utils_vad.py:326-327); the network
 * is causal, so padding further does not change the recording's own probabilities.  The copy is
 * split over `threads` persistent host threads (<= 0: vad_host_threads(), at most 32).  elem_size 1 is a plain
 * byte packing: its zero BYTES are not audio (A-law has no code for 0) -- the staged block goes to the device as it is and
 * vad_upload_rows_coded (how = 2) expands it with the true lengths.                                  */
int  vad_stage_rows(const void *const *rows, const long *lens, long n, long width, size_t elem_size,
                    void *dst, int threads);

/* The same packing WITHOUT a host-side copy, for recordings that already sit in page-locked host memory (hipHostMalloc,
 * torch pin_memory, or vad_host_register below): rows[i] / lens[i] as above, dst = DEVICE [n][width] (16-byte aligned,
 * width * elem_size a multiple of 16).  Asynchronous on `stream`; rows must stay valid until the stream has passed the call.
 *   how = 0  copy engines: one H2D DMA per row (any alignment, no CU time) behind one fill of the batch
 *   how = 1  one gather kernel that reads the rows over PCIe and writes the padded batch (kernel_ingest.hip): a single
 *            launch for any number of rows -- what the continuous-refill scheduler needs (thousands of short rows per slab)
 *   how = 2  rows[] are DEVICE addresses: the recordings were brought over packed, by one large DMA of the arena range
 *            that holds them, and are scattered into the padded batch at HBM speed (the route streams.py takes for a
 *            PackedRecordings whose recordings lie back to back: PCIe carries exactly the live bytes, in big copies)
 * For pageable sources use vad_stage_rows + one copy instead.                                                          */
int  vad_upload_rows(vad_engine *e, const void *const *rows, const long *lens, long n, long width, size_t elem_size,
                     void *dst, int how, void *stream);
/* vad_upload_rows for recordings that are still G.711 (call-centre archives, SIP-trunk recordings: 1 byte a sample): the wire bytes
 * stay as they are in page-locked memory (how = 1) or cross the link in one large DMA of their arena (how = 2), and the gather
 * kernel expands them (the values of vad_g711_expand) on their way into the batch -- half the link bytes of an int16 corpus.
 * lens and width are in SAMPLES; dst = DEVICE int16 [n][width] (16-byte aligned, width a multiple of 8), zero padded behind each
 * row's last sample.  codec_of_row[i] = VAD_PCM_S16 (2 bytes a sample, at an even address), VAD_PCM_ULAW or VAD_PCM_ALAW (1 byte a
 * sample, at ANY byte address: recordings packed back to back move as aligned 16-byte loads all the same); NULL = every row is
 * S16, and so is a table without a G.711 row: the call is then vad_upload_rows(..., elem_size = 2, ...).  The result is, bit for
 * bit, that of vad_upload_rows over the rows expanded by vad_g711_expand.
 * VAD_ERR_ARG, with nothing queued: how = 0 with a G.711 row (a DMA cannot expand), a codec above VAD_PCM_ALAW, lens[i] > width, a
 * null row with a length, a misaligned dst or pitch, an S16 row at an odd address.                                            */
int  vad_upload_rows_coded(vad_engine *e, const void *const *rows, const long *lens, const uint8_t *codec_of_row, long n, long width,
                           void *dst_i16, int how, void *stream);
/* vad_upload_rows_coded for recordings that are still INTERLEAVED -- a recorded call is one file with the agent on the left channel and
 * the customer on the right, frame by frame, G.711 or 16-bit PCM: the data chunk stays as it lies on disk in page-locked memory
 * (how = 1) or crosses the link in one large DMA of its arena (how = 2), once, and the gather kernel writes one batch row per wanted
 * channel.  Source i is frames[i] frames of channels_of_row[i] (1 ... VAD_MAX_CHANNELS; NULL = every source has 1) samples each in
 * format codec_of_row[i] (NULL = every source is S16) at rows[i]: any byte address for G.711, any EVEN address for S16 (a stereo frame
 * may sit at 2 mod 4).  dst_row[VAD_MAX_CHANNELS * i + c] is the row of dst = DEVICE int16 [n_dst][width] (16-byte aligned, width a
 * multiple of 8; frames and width in FRAMES = samples of one channel) that channel c goes to, or -1 for a channel nobody wants.  That
 * row becomes vad_deinterleave(codec_i, channels_i, c, rows[i], frames[i]) followed by int16 zeros to `width`, bit for bit; rows of dst
 * that no entry names are not touched.  With every source at one channel and dst_row[2 i] = i the batch is that of
 * vad_upload_rows_coded.  how = 1 or 2 as in vad_upload_rows.
 * No engine: VAD_ERR_ARG; a host-only engine: VAD_ERR_NO_DEVICE, before the rows are looked at.  VAD_ERR_ARG, with nothing queued and
 * the batch untouched: how = 0 (a DMA neither expands nor splits), a codec above VAD_PCM_ALAW, a channel count outside
 * 1 ... VAD_MAX_CHANNELS, a dst_row entry below -1 or >= n_dst, a batch row named twice, an entry other than -1 for a channel the
 * source does not have, frames[i] > width, a null row with a length, an S16 source at an odd address, a misaligned dst or pitch.   */
#define VAD_MAX_CHANNELS 2
int  vad_upload_rows_channels(vad_engine *e, const void *const *rows, const long *frames, const uint8_t *codec_of_row,
                              const uint8_t *channels_of_row, const int32_t *dst_row /* [n][VAD_MAX_CHANNELS] */,
                              long n, long n_dst, long width, void *dst_i16, int how, void *stream);
/* host twin, re-entrant: channel `channel` of `frames` interleaved frames -> out[0 .. frames) int16 (G.711 expanded: the values of
 * vad_g711_expand); returns frames, or -VAD_ERR_ARG (bad codec, channels not 1 .. VAD_MAX_CHANNELS, channel out of range, frames < 0, NULL with frames > 0) */
long vad_deinterleave(int codec, int channels, int channel, const void *in, long frames, int16_t *out);
/* Page-lock / unlock a host range so that it can be a vad_upload_rows source (hipHostRegister; a decoder's output
 * buffers, a memory-mapped corpus shard).  Process-wide.                                                              */
int  vad_host_register(void *p, size_t bytes);
int  vad_host_unregister(void *p);

/* ---- resampling to the net's rate ---------------------------------------------------------------------------------------------
 * The reference's front door, read_audio(path, sampling_rate) (src/silero_vad/utils_vad.py:138-172), brings a 44.1 / 22.05 / 24 /
 * 11.025 kHz file to the model's rate with torchaudio's default Resample: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99.
 * That function, as arithmetic (not torchaudio's bits): g = gcd(src, dst), O = src / g, N = dst / g, base = min(O, N) * 0.99,
 * W = ceil(6 O / base); for phase j in [0, N) and tap i in [0, 2 W + O)
 *     t = clamp((-j / N + (i - W) / O) * base, -6, 6),   h[j][i] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(t pi / 12)^2 * base / O,
 * evaluated in double and rounded to float32; with the input x (float32, or int16 / 32768) taken as zero outside [0, n),
 *     out[q N + j] = sum_i h[j][i] x[q O + i - W],   cut to ceil(N n / O) samples.
 * The clamp makes every tap outside one short run per phase exactly 0.0f; the table holds that run only: first[j], its first dense
 * tap, and K taps, K the longest run of the pair (a shorter run is followed by 0.0f).  44100 -> 16000: O 441, N 160, W 17, K 34.
 * Served: dst 8000 or 16000, src != dst, O <= 1024, N <= 1024, K <= 160 (88200 -> 8000 has K 134, 11025 -> 16000 has N 640; the
 * caps bound the table and keep the span of input one tile of the kernel stages in LDS under 64 KiB).  Any other pair is
 * VAD_ERR_SAMPLE_RATE.  NOT the same thing as a forward call's sr = 32000 / 48000: that is the reference's x[::k] inside the model
 * (no low-pass); src = 48000 here is read_audio's low-pass resample.  Both exist in the reference.
 * Non-finite samples poison the outputs whose K stored taps cover them; a dense convolution would poison the whole 2 W + O window
 * (0 * NaN).  That is not emulated.
 * The first four and the three vad_resample_stream_* calls need no engine and no GPU.                                             */
int  vad_resample_geometry(int src, int dst, int *O, int *N, int *W, int *K);      /* any pointer may be NULL */
/* ceil(N n / O): the samples n input samples become; -VAD_ERR_SAMPLE_RATE, -VAD_ERR_ARG (n < 0) */
long vad_resample_length(int src, int dst, long n);
/* The pair's table, the ONE source of it for the device, the host twin and Python: taps[N][K] row-major, first[N]. */
int  vad_resample_table(int src, int dst, float *taps /* [N][K] */, int32_t *first /* [N] */);
/* host twin, re-entrant: n samples of elem_size 2 (int16) or 4 (float32) at pcm -> out[0 .. vad_resample_length(src, dst, n)); the
 * same table, every sum accumulated in double over the K stored taps in order and rounded once to float32. */
int  vad_resample_host(int src, int dst, const void *pcm, size_t elem_size, long n, float *out);
/* THE STREAMING FORM of the same function, for a signal that arrives in pieces (the pump's resampled rows; host only, re-entrant).
 * Output m = q N + j reads the K inputs p0 ... p0 + K - 1, p0 = q O + first[j] - W, inputs before 0 being zero.  A stream that has
 * received g input samples has emitted exactly the outputs with p0 + K <= g: "ready(g)".  Nothing is zero-extended on the right, so an
 * emitted output never changes and equals, for every cut of the signal into pieces, the output of the whole signal.  p0 + K does not
 * fall from one output to the next (first[] is non-decreasing and first[N - 1] <= first[0] + O: checked when the table is made, and a
 * pair that failed it would have no streaming form, -VAD_ERR_SAMPLE_RATE), so the emitted outputs are a prefix and ready(g) is a count;
 * it is non-decreasing in g, at most ceil(N g / O), and ready(g + O) = ready(g) + N once g + O >= first[N - 1] - W + K.  The latency,
 * the inputs behind an output's nominal position floor(m O / N) that must arrive before it is emitted, is at most max_j (first[j] -
 * floor(j O / N)) - W + K: 19 input samples for 44.1 -> 16 kHz and 48 -> 16 kHz, 11 for 24 -> 16 kHz, 10 for 22.05 -> 16 kHz, 35 for
 * 44.1 -> 8 kHz.
 * vad_resample_stream_ready: ready(g); -VAD_ERR_SAMPLE_RATE for a pair that is not served, -VAD_ERR_ARG for g < 0.  Exact for g up to
 * 2^40 and far beyond: whole periods (O inputs for N outputs) are taken out of g first, everything is 64-bit.
 * vad_resample_stream_history: H, the input samples a stream must keep so that every output not yet emitted finds its K inputs in
 * history ++ the next piece.  H = K - 1.  Derivation: an output m that is not emitted at g has p0(m) + K > g, i.e. p0(m) >= g - (K - 1),
 * so no unemitted output reads further back than K - 1 samples; and the bound is met whenever a piece ends at g = p0(m) + K - 1 for a
 * phase whose run has all K taps, so K - 2 samples are not enough (tests/test_pump_resample.py).  (K + (dhi - dlo) + ceil(O / N), with
 * dlo / dhi the extremes of first[j] - floor(j O / N), also suffices, but it bounds the spread of the phases a second time: the rule
 * above already says where every unemitted output starts.)  < 0: -VAD_ERR_SAMPLE_RATE.
 * vad_resample_stream_host: the host twin of one piece.  g = the inputs the stream received before it, history[H] = the last H of them,
 * oldest first, zeros where the stream has not lived that long; in[n] = the piece.  Writes the outputs ready(g) ... ready(g + n) - 1 to
 * out (accumulated as vad_resample_host does: double, tap order, one rounding -- bit for bit its outputs of the whole signal) and, if
 * history_out is not NULL, the next piece's history (history_out may be history).  Returns their number, ready(g + n) - ready(g), or
 * -VAD_ERR_SAMPLE_RATE / -VAD_ERR_ARG (g < 0, n < 0, a NULL history, a NULL piece with n > 0, a NULL out with an output due).         */
long vad_resample_stream_ready(int src, int dst, long g);
int  vad_resample_stream_history(int src, int dst);
long vad_resample_stream_host(int src, int dst, long g, const int16_t *history, const int16_t *in, long n, float *out, int16_t *history_out);
/* The device route: pcm = DEVICE [n][ld] at rate src, elem_size 2 or 4; lens[r] = live samples of row r, a device-visible table
 * (device or page-locked memory, like vad_upload_rows' row table) that must stay valid until the stream has passed the call;
 * dst_buf = DEVICE float32 [n][ldd], ldd >= width_out.  Sample m of row r is the sum above for m < ceil(N lens[r] / O) and exactly
 * 0.0f from there to width_out (the reference cuts the resampled signal, then audio_forward zero-pads its last chunk).  A row ends
 * at lens[r] (clamped to [0, ld]): the batch behind it is not read, whatever it holds.  fp32 accumulation in tap order, a function
 * of the output index alone: a recording gives the same bits in any row of any batch at any pitch; each output is within
 * (K + 1) 2^-24 sum_k |h_k x_k| of vad_resample_host's.  Asynchronous on `stream`, no synchronisation; nothing is allocated once
 * the pair's table is on the device -- vad_resample_reserve puts it there up front (beside vad_reserve; an engine and its clones
 * share the tables), otherwise the first call of a pair does, with two blocking copies.                                          */
int  vad_resample_reserve(vad_engine *e, int src, int dst);
int  vad_resample_rows_device(vad_engine *e, int src, int dst, const void *pcm, size_t elem_size, long ld, const long *lens, long n,
                              long width_out, float *dst_buf, long ldd, void *stream);

/* The continuous-refill schedule of silero_vad_amd/streams.py RefillPlan (the reference's padded lock-step batch, tuning/utils.py:146-160,
 * with rows retired and re-admitted): recording q (in admission order) occupies a stream slot for need[q] time slabs; at every slab
 * boundary every free slot, lowest first, takes the next recording.  Writes the slab at which q is admitted and its slot.  Host only. */
int  vad_refill_schedule(const long *need, long n, long slots, long *start, long *slot);
/* ... and the schedule as the table the stager walks: one row of five longs per (recording, slab it is active in) -- slot, recording,
 * first sample, samples, reset flag -- ordered by slab, then by slot; cuts[k] .. cuts[k + 1] (n_slabs + 1 entries) are slab k's rows.
 * Queue entry q is recording rec[q] of len[q] samples; width = samples per slab; rows has room for sum(need) rows.  Returns the number
 * of rows, or -VAD_ERR_ARG.  Host only.                                                                                           */
long vad_refill_table(const long *need, const long *start, const long *slot, const long *rec, const long *len, long n, long slots,
                      long width, long n_slabs, long *rows, long *cuts);

/* Do two streams of the engine's device run BESIDE each other?  The HIP runtime maps streams onto a handful of hardware queues
 * (GPU_MAX_HW_QUEUES, 4 by default; which stream lands where depends on the order in which the process' streams were first
 * used), and two streams on one queue execute their kernels one after the other whatever the events say.  A pipeline that wants
 * its upload kernel beside its compute kernels (vad_upload_rows how = 1 on one stream, vad_forward_audio on another) asks before
 * it commits to a pair of streams, and takes another stream if the answer is 0 (silero_vad_amd/streams.py does).  Returns 1: a
 * short kernel on b finished while a ~1 ms kernel on a was still running; 0: it waited for it; < 0: -vad_status.  Synchronises
 * both streams; costs ~1 ms.                                                                                                */
int  vad_streams_overlap(vad_engine *e, void *stream_a, void *stream_b);

/* Host threads the native helpers (vad_stage_rows, vad_segment_probs_batch) use by default in THIS process:
 * min(CPU affinity, cgroup CPU quota) / LOCAL_WORLD_SIZE, i.e. the node's CPU budget divided among the one-process-per-GPU
 * ranks torchrun started (SILERO_VAD_AMD_HOST_THREADS overrides).                                                     */
int  vad_host_threads(void);
/* Narrow the calling thread's CPU affinity to the CPUs of `device`'s NUMA node (threads and pinned buffers created
 * afterwards follow).  Returns the node, or -1 if it is unknown or outside the process' CPU mask (nothing changed).   */
int  vad_bind_host_to_device(int device);

/* ---- decoder training -------------------------------------------------------------------------------------------------------------
 * The reference's train() (tuning/utils.py:206-249, driven by tune.py) learns one module, VADDecoderRNNJIT: LSTMCell(128, 128),
 * Dropout, ReLU, Conv1d(128, 1, 1), Sigmoid -- 132 225 parameters -- on the output of the frozen STFT and encoder, with the loss
 * (BCELoss(reduction = 'none') * masks).mean() over the padded batch.  Three calls bring that to the device.
 *
 * vad_encode_audio: feat[b][t][0..127] = ReLU output of encoder 3 for chunk t of row b, what the reference's stft + encoder return.
 * pcm (elem_size 2 = int16 or 4 = float32, [B][ld]), ctx ([B][64 | 32], read only: every row starts from the context given and the
 * next context is dropped) and feat ([B][T][128], T = ceil(ceil(L / k) / N), 16-byte aligned) are device pointers.  sr as for
 * vad_forward_audio: 8000, 16000 or a multiple of 16000, decimated the same way; long inputs run in the same time slabs.  The values
 * are the bits of the operand the product's gate GEMM consumes; a non-finite sample makes its chunk's vector NaN.
 * The first call builds a second set of weight images (two blocking copies, one device synchronisation); after that nothing is
 * allocated beyond the engine's scratch (vad_reserve).  Asynchronous on `stream`.  Not with impl=reference (VAD_ERR_OPTION).        */
int vad_encode_audio(vad_engine *e, int sr, int B, long L, const void *pcm, size_t elem_size, long ld, const float *ctx, float *feat,
                     void *stream);

/* Loss and gradients of the decoder by back-propagation through time.  The rule (csrc/trainer.hpp): row b runs from zero (h, c)
 * over t < n_chunks[b], nothing behind that is read; aten::lstm_cell in gate order i, f, g, o; y = keep ? relu(h) keep_scale : 0
 * (keep == NULL: y = relu(h)); z = w_out y + b_out; p = sigmoid(z).  Chunk weight w: 1 for label 1, noise_loss for label 0, 0 for
 * any other label (VAD_LABEL_IGNORE).  loss = sum w bce(p, label) / denom with nn.BCELoss's term (log clamped at -100, taken in
 * double); for a batch of the reference denom = len(batch) * longest row.  The head's backward is on the float32 probability,
 * dz = (w / denom) (p - label) [p (1 - p) / max(p (1 - p), 1e-12)]: a chunk whose fp32 p is exactly 0 or 1 hands back nothing, as
 * under torch.  The rest is plain BPTT; db_ih and db_hh are the same sums.
 * Shapes: w_ih, w_hh [512][128]; b_ih, b_hh [512]; w_out [128]; b_out [1]; feat [B][T][128]; labels [B][ldl], ldl >= T;
 * keep [B][T][128] bytes (0 = dropped) or NULL; probs [B][T] or NULL (0 behind n_chunks).
 * Device call: every pointer is a device pointer; asynchronous on `stream`, allocates nothing; fp32 with the ulp-accurate
 * activations of csrc/activations.hpp; no float atomics -- the same inputs give the same bits, and a row's probabilities do not depend on its place
 * in the batch.  Workspace: vad_decoder_grad_workspace_bytes(B, T) bytes, 256-byte aligned, about B T (512 * 2 + 7 * 128) * 4 bytes
 * plus at most 34 MB of split-K slabs (280 MB in all at 128 x 250); 0 = B T out of range.  n_chunks[b] is clamped to [0, T].
 * VAD_ERR_ARG, with nothing queued and nothing written: a NULL pointer, B <= 0, T <= 0, ldl < T, denom <= 0 (or NaN), feat / w_ih /
 * w_hh not 16-byte aligned, any other tensor not 4-byte aligned, loss / n_chunks not 8-byte aligned, a workspace that is not
 * 256-byte aligned or too small.  A host-only engine: VAD_ERR_NO_DEVICE.
 * Host twin: no engine, host pointers, everything in double except that p is rounded to float32 before the loss term and dz; the
 * parameters and the gradients are DOUBLE (the reference the device call and the fixtures are compared with); n_chunks[b] outside
 * [0, T] is VAD_ERR_ARG.  The result does not depend on `threads` (<= 0: vad_host_threads(), at most 64).                          */
typedef struct { const float *w_ih, *w_hh, *b_ih, *b_hh, *w_out, *b_out; } vad_decoder_params;
typedef struct { float *w_ih, *w_hh, *b_ih, *b_hh, *w_out, *b_out; } vad_decoder_grads;
typedef struct { const double *w_ih, *w_hh, *b_ih, *b_hh, *w_out, *b_out; } vad_decoder_params_f64;
typedef struct { double *w_ih, *w_hh, *b_ih, *b_hh, *w_out, *b_out; } vad_decoder_grads_f64;
size_t vad_decoder_grad_workspace_bytes(int B, long T);
int vad_decoder_grad_device(vad_engine *e, const vad_decoder_params *p, const float *feat, int B, long T, const long *n_chunks,
                            const uint8_t *labels, long ldl, const uint8_t *keep /* [B][T][128] or NULL */, float keep_scale,
                            float noise_loss, double denom, vad_decoder_grads *g, double *loss, float *probs /* [B][T] or NULL */,
                            void *workspace, size_t workspace_bytes, void *stream);
int vad_decoder_grad_host(const vad_decoder_params_f64 *p, const float *feat, int B, long T, const long *n_chunks, const uint8_t *labels,
                          long ldl, const uint8_t *keep, float keep_scale, float noise_loss, double denom, vad_decoder_grads_f64 *g,
                          double *loss, float *probs, int threads);

/* ---- AUDIO AUGMENTATION of training batches (the rule: csrc/augment.hpp) ------------------------------------------------------------
 * The reference trains on audiomentations' SomeOf((1, 3)) of fifteen transforms; the ten with arithmetic that can be stated are three
 * op kinds here.  A row's recipe is an ordered list of 0 .. 3 ops, each applied to the float32 output of the one before:
 *   VAD_AUGMENT_NOISE    y[n] = x[n] + float(a) g(seed, row_key, n), g standard normal from Philox4x32-10 (key = seed, counter =
 *                        (n / 4, row_key)) through Box-Muller in double: a sample's noise depends on (seed, row_key, n) alone.
 *   VAD_AUGMENT_BIQUADS  n_sections (1 .. 8) second-order sections coef[s] = b0 b1 b2 a1 a2 (a0 = 1), zero initial state, the
 *                        recursion in DOUBLE on the device as in the twin, rounded to float32 once: scipy.signal.sosfilt's function.
 *   VAD_AUGMENT_CLIP     lo, hi = the a- and b-quantile (0 <= a <= b <= 1) of the row's own len samples, numpy's default method in
 *                        double (exact order statistics), rounded to float32; y = x < lo ? lo : x > hi ? hi : x.
 * pcm [n][ld]: int16 (elem_size 2, taken as x / 32768) or float32 (elem_size 4).  out [n][ld_out] float32, 16-byte aligned, ld_out a
 * multiple of 4, not overlapping pcm: row i is written over its whole ld_out, zero at and behind lens[i].  A row whose final result
 * holds a non-finite value comes back as its input converted to float32, bit for bit; so does a row whose recipe is empty.
 * Device call: every pointer but the engine is a device pointer; asynchronous on `stream`, allocates nothing, no float atomics: the
 * same call gives the same bits and a row's output does not depend on its place in the batch.  lens[i] is clamped to
 * [0, min(ld, ld_out)].  The recipes are device memory the call cannot read: a row whose recipe vad_augment_check_recipes would refuse
 * comes back as its input.  Workspace: vad_augment_workspace_bytes(n, ld_out) bytes, 256-byte aligned (0 = out of range): 128 bytes
 * per block of vad_augment_block() samples.  VAD_ERR_ARG with nothing queued: a NULL pointer, n <= 0, ld or ld_out <= 0, elem_size
 * not 2 or 4, a misaligned pointer, ld_out not a multiple of 4, a workspace too small.  A host-only engine: VAD_ERR_NO_DEVICE.
 * Host twin: host pointers, no alignment rule; the same function, not the same block structure; the result does not depend on
 * `threads` (<= 0: vad_host_threads(), at most 64).  VAD_ERR_ARG: the above, a lens[i] outside [0, min(ld, ld_out)], and a recipe
 * that vad_augment_check_recipes refuses.
 * vad_augment_check_recipes (host memory): VAD_OK, or VAD_ERR_ARG with *why (may be NULL) set to a static sentence: n_ops outside
 * 0 .. 3, n_sections outside 1 .. 8, a non-finite coefficient or amplitude, quantiles outside 0 <= a <= b <= 1, an unknown kind.
 * vad_biquad_design (host, double): one Audio-EQ-cookbook (R. Bristow-Johnson) section normalised to a0 = 1.  12 dB/oct Butterworth
 * low- and high-pass are one section at q = 1/sqrt(2); 24 dB/oct two sections at q = 1 / (2 cos(pi / 8)), 1 / (2 cos(3 pi / 8)) = 0.54119610, 1.30656296.  Band-pass has 0 dB
 * peak gain; gain_db is read by peaking and the shelves only (q is the shelves' Q, not a slope).  VAD_ERR_ARG: an unknown kind,
 * sr <= 0, f0 outside (0, sr / 2), q <= 0, a non-finite argument.
 *
 * Room reverb and aliasing (two more of the fifteen; AirAbsorption, Mp3Compression and PitchShift stay out), through the _x entry points:
 *   VAD_AUGMENT_FIR      n_sections = K taps (1 .. VAD_AUGMENT_MAX_TAPS), seed = index of tap 0 in a float32 bank that travels beside
 *                        the recipes: y[n] = sum over k = 0 .. min(n, K - 1) of h[k] x[n - k], causal from zero state, the output as
 *                        long as the input (audiomentations' ApplyImpulseResponse / RoomSimulator with leave_length_unchanged).  Direct
 *                        form: the twin sums exact products in double in ascending k and rounds once; the device runs a float32
 *                        multiply-add chain in an order that depends on (K, n) alone, |device - twin| <= (K + 2) 2^-24 sum |h||x|; a
 *                        zero tap adds exactly nothing and digital silence longer than K stays exactly zero.
 *   VAD_AUGMENT_ALIAS    a = new sample rate, b = the row's, 0 < a <= b: audiomentations' Aliasing, two np.interp calls on
 *                        linspace grids, numpy's statements in double (csrc/augment.hpp), rounded to float32 once; bit-equal on both
 *                        sides.  len < 2 or round(len a / b) < 2 leaves the row as it is.
 * vad_augment_extra is host memory read at the call; its pointers are device pointers for the device call: the bank (4-byte aligned,
 * may be NULL with fir_bank_len 0) and the second row buffer both ops need (16-byte aligned, vad_augment_scratch_bytes(n, ld_out)
 * bytes; 0 = out of range), separate from the workspace.  vad_augment_rows_device_x with extra == NULL is vad_augment_rows_device;
 * the entry points without _x treat FIR and ALIAS as unknown kinds and queue none of their launches.  A FIR whose range
 * [seed, seed + K) leaves the bank: the device returns the row as its input, the twin and the check refuse it.  Otherwise the _x
 * calls keep the contract above; VAD_ERR_ARG with nothing queued also for a NULL or misaligned scratch, a scratch too small, a
 * misaligned bank, fir_bank_len < 0 or a NULL bank with fir_bank_len > 0.
 * vad_augment_check_recipes_bank: vad_augment_check_recipes that accepts the two kinds against a bank of bank_len taps; further
 * sentences: taps outside 1 .. 8192, taps outside the bank, rates outside 0 < a <= b.
 * vad_rir_shoebox (host, double): Allen and Berkley's image-source response of a box room, a STATED rule in the spirit of
 * RoomSimulator, not pyroomacoustics' bits.  beta = sqrt(1 - absorption), c = 343 m/s, d0 = |src - mic|; for nx, ny, nz in
 * [-max_order, max_order] and px, py, pz in {0, 1}, in that nesting order: image coordinate 2 n L + (1 - 2 p) src per axis,
 * R = sum |n - p| + |n| (skipped if R > max_order), d its distance to the microphone, amplitude A = beta^R d0 / d (0^0 = 1), delay
 * t = (d - d0) sr / c samples, j = floor(t), f = t - j: h[j] += A (1 - f), h[j + 1] += A f where the index is below n_taps; sums in
 * double, written as float32.  The direct sound is tap 0 with gain 1: the flight time is taken out, so labels stay aligned.
 * VAD_ERR_ARG: a NULL pointer, a non-finite argument, sr or a room size <= 0, a position not strictly inside the room, src == mic,
 * absorption outside (0, 1], max_order < 0, n_taps outside 1 .. 8192.                                                                */
#define VAD_AUGMENT_MAX_OPS 3
#define VAD_AUGMENT_MAX_SECTIONS 8
#define VAD_AUGMENT_MAX_TAPS 8192
enum { VAD_AUGMENT_NOISE = 1, VAD_AUGMENT_BIQUADS = 2, VAD_AUGMENT_CLIP = 3, VAD_AUGMENT_FIR = 4, VAD_AUGMENT_ALIAS = 5 };
enum { VAD_BIQUAD_LOWPASS = 0, VAD_BIQUAD_HIGHPASS = 1, VAD_BIQUAD_BANDPASS = 2, VAD_BIQUAD_NOTCH = 3, VAD_BIQUAD_PEAKING = 4,
       VAD_BIQUAD_LOWSHELF = 5, VAD_BIQUAD_HIGHSHELF = 6 };
typedef struct {
    int32_t kind;                                   /* VAD_AUGMENT_*                                     */
    int32_t n_sections;                             /* BIQUADS; FIR: the number of taps                  */
    double coef[VAD_AUGMENT_MAX_SECTIONS][5];       /* BIQUADS: b0 b1 b2 a1 a2                           */
    double a, b;                                    /* NOISE: a = amplitude; CLIP: a = q_lo, b = q_hi; ALIAS: a = new rate, b = rate */
    uint64_t seed;                                  /* NOISE; FIR: index of the first tap in the bank    */
} vad_augment_op;
typedef struct {
    int32_t n_ops;
    int32_t reserved;
    vad_augment_op ops[VAD_AUGMENT_MAX_OPS];
    uint64_t row_key;
} vad_augment_recipe;
long vad_augment_block(void);
size_t vad_augment_workspace_bytes(long n_rows, long width);
int vad_augment_check_recipes(const vad_augment_recipe *recipes, long n, const char **why);
int vad_augment_rows_device(vad_engine *e, const void *pcm, size_t elem_size, long ld, const long *lens, long n,
                            const vad_augment_recipe *recipes, float *out, long ld_out, void *workspace, size_t workspace_bytes,
                            void *stream);
int vad_augment_rows_host(const void *pcm, size_t elem_size, long ld, const long *lens, long n, const vad_augment_recipe *recipes,
                          float *out, long ld_out, int threads);
int vad_biquad_design(int kind, double sr, double f0, double q, double gain_db, double coef[5]);
typedef struct {
    const float *fir_bank;                          /* [fir_bank_len] taps, or NULL                      */
    long fir_bank_len;
    void *scratch;                                  /* vad_augment_scratch_bytes(n, ld_out) bytes        */
    size_t scratch_bytes;
} vad_augment_extra;
size_t vad_augment_scratch_bytes(long n_rows, long width);
int vad_augment_check_recipes_bank(const vad_augment_recipe *recipes, long n, long bank_len, const char **why);
int vad_augment_rows_device_x(vad_engine *e, const void *pcm, size_t elem_size, long ld, const long *lens, long n,
                              const vad_augment_recipe *recipes, float *out, long ld_out, void *workspace, size_t workspace_bytes,
                              const vad_augment_extra *extra, void *stream);
int vad_augment_rows_host_x(const void *pcm, size_t elem_size, long ld, const long *lens, long n, const vad_augment_recipe *recipes,
                            float *out, long ld_out, const float *fir_bank, long fir_bank_len, int threads);
int vad_rir_shoebox(double sr, const double room[3], const double src[3], const double mic[3], double absorption, int max_order,
                    float *h, long n_taps);

/* ---- RESIDENT TRAINING: batches cut out of a corpus in HBM, Adam on the device (the rules: csrc/trainset.hpp) -----------------------
 * A tuning corpus is small beside HBM and is visited once per epoch: it is uploaded once, as one arena of int16 or float32 samples
 * (elem_size 2 or 4) with recording r at arena[offs[r] .. offs[r] + lens[r]) and its per-chunk labels at label_arena[label_offs[r] ..),
 * and every batch is assembled where it lies.  Row b takes recording r = idx[b]:
 *     len = min(lens[r], max_samples),  out_pcm[b][0 .. len) = the recording's first len samples in the arena's element type, exact
 *     zeros from len to ld;  out_n_chunks[b] = ceil(len / chunk);  out_labels[b][t] = the recording's label for t < n_chunks,
 *     VAD_LABEL_IGNORE from there to ldl;  out_lens[b] = len.
 * Every output is written over its whole pitch, whatever it held.  offs, lens, label_offs, idx, out_lens and out_n_chunks are longs.
 * Device call: every pointer but the engine is a device pointer; stateless, allocates nothing, asynchronous on `stream`, one launch,
 * no atomics: a row's bytes depend on its recording alone, not on its place in the batch.  A recording may start at ANY
 * element-aligned address (even for int16, 4-byte for float32): 16-byte vectors where source and destination allow, elements
 * otherwise, the same bytes either way.  The call cannot read the tables: an idx[b] outside [0, n_recordings) gives an empty row (len
 * 0, zeros, VAD_LABEL_IGNORE), and a cut longer than ld (or its chunks than ldl) is cut at the pitch, never written past it.
 * VAD_ERR_ARG with nothing queued: a NULL pointer, elem_size not 2 or 4, n_recordings, B, chunk, ld or ldl <= 0, max_samples < 0, a
 * sample pointer that is not element-aligned, a table that is not 8-byte aligned.  A host-only engine: VAD_ERR_NO_DEVICE.
 * Host twin: host pointers, no engine; VAD_ERR_ARG besides: an idx[b] outside [0, n_recordings), a negative length, ld < a row's
 * len, ldl < a row's n_chunks -- nothing is written then.
 *
 * vad_decoder_adam_device: torch.optim.Adam's default rule (no amsgrad, no weight decay, not maximize) over the six decoder tensors,
 * 132 225 parameters, in one launch, in float32 in the order of torch's composed operations:
 *     m = m + (g - m)(1 - beta1),  v = beta2 v + (1 - beta2) g g,  p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * params (written), m and v (state, written) are vad_decoder_grads-shaped, grads (read) vad_decoder_params-shaped, device pointers,
 * 4-byte aligned.  The bias corrections are taken on the host in double from `step` and passed as kernel arguments: there is no
 * counter on the device, the caller counts.  step == 1 starts the state: m and v are zeroed by a launch in front (they count as
 * zero whatever they held); no later step touches them but through the rule.  A non-finite gradient propagates, as under torch.
 * Stateless, allocates nothing, asynchronous on `stream`.  VAD_ERR_ARG with nothing queued: a NULL pointer, a misaligned tensor,
 * step < 1, beta1 or beta2 outside [0, 1), lr or eps negative or NaN.
 * Host twin: double parameters, gradients and state (as vad_decoder_grad_host takes double parameters), the same rule in double.      */
int vad_trainset_batch_device(vad_engine *e, const void *arena, size_t elem_size, const long *offs, const long *lens,
                              const uint8_t *label_arena, const long *label_offs, long n_recordings, const long *idx, long B,
                              long max_samples, long chunk, void *out_pcm, long ld, uint8_t *out_labels, long ldl, long *out_lens,
                              long *out_n_chunks, void *stream);
int vad_trainset_batch_host(const void *arena, size_t elem_size, const long *offs, const long *lens, const uint8_t *label_arena,
                            const long *label_offs, long n_recordings, const long *idx, long B, long max_samples, long chunk,
                            void *out_pcm, long ld, uint8_t *out_labels, long ldl, long *out_lens, long *out_n_chunks);
int vad_decoder_adam_device(vad_engine *e, const vad_decoder_grads *params, const vad_decoder_params *grads, const vad_decoder_grads *m,
                            const vad_decoder_grads *v, long step, double lr, double beta1, double beta2, double eps, void *stream);
int vad_decoder_adam_host(const vad_decoder_grads_f64 *params, const vad_decoder_params_f64 *grads, const vad_decoder_grads_f64 *m,
                          const vad_decoder_grads_f64 *v, long step, double lr, double beta1, double beta2, double eps);

/* ---- test / bring-up hooks (not part of the drop-in surface) -------------------------------------
 * Host-only: size and contents of the packed weight images the kernels consume, so CPU tests can
 * check the fragment packing without a GPU.  which: 0 = frontend GEMM stream (enc0 "direct"), 1 = recurrent
 * W_hh image, 2 = small tables (biases, head, window, twiddles), 5 = frontend stream in Winograd F(2,3) form,
 * 6 = frontend stream in Winograd F(4,3) form (the product's), 7 = recurrent image as three bf16 pieces per weight
 * (option rec=bf16x9), 8 = the F(4,3) frontend program as three bf16 pieces per weight (option front_mma=bf16x9); 7 and 8 are
 * returned as raw 4-byte words holding two bf16 each.                                                              */
long vad_debug_packed_floats(const vad_engine *e, int sr, int which);
int  vad_debug_packed_copy(const vad_engine *e, int sr, int which, float *dst, long n);
/* Host-only engine for the hooks above (no device needed).                                       */
int  vad_create_host_only(const void *weights, size_t nbytes, vad_engine **out);
/* Device: run the frontend only and return the LSTM input-gate pre-activations
 * gx[B][T][512] = W_ih * enc(stft(x)) + b_ih + b_hh  (row-major, gate order i,f,g,o).            */
int  vad_debug_frontend(vad_engine *e, int sr, int B, long L, const float *pcm, long ld,
                        const float *ctx, float *gx, void *stream);

/* Device: y[i] = sigmoid(x[i]) (kind 0) or tanh(x[i]) (kind 1) exactly as the recurrent kernels evaluate them
 * (v_exp_f32 / v_rcp_f32 based, csrc/activations.hpp); x, y device pointers.  For the accuracy test.        */
int  vad_debug_activation(vad_engine *e, int kind, const float *x, float *y, long n, void *stream);

/* Device: launch a "foreign tenant" on `stream`: `blocks` one-wave workgroups that execute nothing but fp32
 * VALU FMAs for `iters` rounds (kind 0: packed v_pk_fma_f32, kind 1: scalar v_fma_f32).  The GPU tests run
 * it beside the engine's kernels to check their results under a co-resident foreign kernel.  Asynchronous. */
int  vad_debug_foreign_load(vad_engine *e, int kind, int blocks, long iters, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SILERO_VAD_HIP_H */
