// kernel_resample.hip -- recordings at 44.1 / 22.05 / 24 / 11.025 kHz (any rate whose reduced ratio fits the caps below) brought to the
// net's rate on the device: the polyphase FIR of the reference's front door, read_audio(path, sampling_rate), which resamples with
// torchaudio's default Resample (src/silero_vad/utils_vad.py:138-172; sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).
//
// The function.  g = gcd(src, dst), O = src / g, N = dst / g, base = min(O, N) 0.99, W = ceil(6 O / base); for phase j in [0, N) and
// tap i in [0, 2 W + O):  t = clamp((-j / N + (i - W) / O) base, -6, 6),  h[j][i] = sinc(t) cos(t pi / 12)^2 base / O, evaluated in
// double and rounded to float32.  With x zero outside [0, L), output q N + j = sum_i h[j][i] x[q O + i - W], cut to ceil(N L / O)
// samples.  The clamp makes every tap outside one short run per phase exactly 0.0f: the table keeps that run only -- first[j] and K
// taps, K the longest run of the pair, a shorter run followed by 0.0f -- so 44.1 -> 16 kHz is 34 products per output, not 475.
//
//   * ONE source of the table (resample_table below): the device image, the CPU twin vad_resample_host and Python read the same floats;
//   * a workgroup of 256 lanes makes one TILE of kResampleTile (1024) consecutive outputs of one row.  It stages the span of input the
//     tile reads -- floor(m0 O / N) + dlo - W ... floor(m1 O / N) + dhi - W + K, with dlo / dhi the extremes of first[j] - floor(j O / N)
//     -- into LDS as float32 (int16 / 32768 is exact), samples before 0 and from the row's LENGTH on as 0.0f: the row's end comes from
//     the length table, never from what the batch holds behind it, and the inner loop has no bounds to test;
//   * lane t owns outputs m0 + t + 256 i: consecutive lanes, consecutive outputs -- coalesced stores, and consecutive phases: the device
//     image of the table is TRANSPOSED, taps[k][j], so a wave's tap loads are consecutive floats (the table, 21 KB for 44.1 -> 16 kHz,
//     stays in L2 / the vector cache); the LDS reads of a wave step by O / N samples a lane (2.76 for 44.1 -> 16 kHz: 3 lanes a bank);
//   * acc = fmaf(tap k, x k, acc) for k = 0 ... K - 1, fp32, no atomics: the order is a function of the output index alone, so a
//     recording gives the same bits in any row of any batch at any pitch;
//   * outputs from the row's cut ceil(N len / O) to width_out are written as 0.0f (the reference cuts the resampled signal, then
//     audio_forward zero-pads its last chunk); a tile wholly behind the cut stages nothing.
// Footprint: no MFMA, a few dozen VGPRs, LDS = the span (11 KB for 44.1 -> 16 kHz, under 64 KB at the caps).  It runs on a compute
// lane's stream in front of that lane's frontend and beside the other lane's kernels; a tile lives for microseconds, so it does not
// hold SIMDs against the frontend's 243-VGPR waves the way a persistent wide gather did (kernel_ingest.hip).
//
// Non-finite samples poison the outputs whose stored run of K taps covers them; a dense convolution (torchaudio's conv1d) would
// poison the whole 2 W + O window through 0 * NaN.  That is not emulated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "device_api.hpp"

namespace vad {

namespace {

long gcd_l(long a, long b) {
    while (b) {
        const long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

std::mutex g_table_mutex;
std::map<std::pair<int, int>, std::shared_ptr<const ResampleHostTable>> g_tables;     // (src, dst) -> table, served pairs only

std::shared_ptr<const ResampleHostTable> build_table(int src, int dst) {
    if ((dst != 8000 && dst != 16000) || src <= 0 || src == dst) return nullptr;
    const long g = gcd_l(src, dst);
    const long O = src / g, N = dst / g;
    if (O > kResampleMaxRatio || N > kResampleMaxRatio) return nullptr;
    const double pi = 3.14159265358979323846;
    const double base = (double)(O < N ? O : N) * 0.99;
    const long W = (long)std::ceil(6.0 * (double)O / base);
    if (2 * W + 1 > 2 * kResampleMaxTaps) return nullptr;             // (K is about 2 W (1 + ...): far above the cap, before the table is made)
    const long D = 2 * W + O;
    auto t = std::make_shared<ResampleHostTable>();
    std::vector<float> h((size_t)D);
    std::vector<long> lo((size_t)N), cnt((size_t)N);
    std::vector<std::vector<float>> runs((size_t)N);
    long K = 0;
    for (long j = 0; j < N; ++j) {
        long a = -1, b = -1;
        for (long i = 0; i < D; ++i) {
            double x = (-(double)j / (double)N + (double)(i - W) / (double)O) * base;
            x = x < -6.0 ? -6.0 : x > 6.0 ? 6.0 : x;
            const double c = std::cos(x * pi / 6.0 / 2.0);
            const double win = c * c;
            const double xp = x * pi;
            const double s = xp == 0.0 ? 1.0 : std::sin(xp) / xp;
            h[(size_t)i] = (float)(s * win * (base / (double)O));
            if (h[(size_t)i] != 0.0f) {
                if (a < 0) a = i;
                b = i;
            }
        }
        if (a < 0) return nullptr;                                   // (a phase without a tap: no pair within the caps has one)
        lo[(size_t)j] = a;
        cnt[(size_t)j] = b - a + 1;
        runs[(size_t)j].assign(h.begin() + a, h.begin() + b + 1);
        K = std::max(K, b - a + 1);
    }
    if (K > kResampleMaxTaps) return nullptr;
    t->g = ResampleGeom{(int)O, (int)N, (int)W, (int)K, 0, 0, 0};
    t->taps.assign((size_t)(N * K), 0.0f);
    t->first.resize((size_t)N);
    long dlo = 0, dhi = 0;
    for (long j = 0; j < N; ++j) {
        t->first[(size_t)j] = (int32_t)lo[(size_t)j];
        for (long k = 0; k < cnt[(size_t)j]; ++k) t->taps[(size_t)(j * K + k)] = runs[(size_t)j][(size_t)k];
        const long a = lo[(size_t)j] - j * O / N;                     // first[j] - floor(j O / N)
        if (j == 0 || a < dlo) dlo = a;
        if (j == 0 || a > dhi) dhi = a;
    }
    t->g.dlo = (int)dlo;
    t->g.dhi = (int)dhi;
    // the longest span a tile stages: floor((tile - 1) O / N) + 1 input positions between its first and last output, the spread of
    // first[] around j O / N, and the K taps of the last one
    const long span = (long)(kResampleTile - 1) * O / N + 1 + (dhi - dlo) + K;
    if (span * (long)sizeof(float) > 65536) return nullptr;
    t->g.span = (int)span;
    // the streaming rule: output q N + j is emitted once q O + end[j] inputs have arrived.  It is a COUNT only if that figure never
    // falls from one output to the next, inside a period and across its boundary; every pair within the caps passes (tests/test_pump_resample.py)
    bool counts = true;
    for (long j = 0; j < N; ++j) {
        const long e = lo[(size_t)j] - W + K;
        counts = counts && (j == 0 || e >= lo[(size_t)j - 1] - W + K);
    }
    counts = counts && lo[(size_t)N - 1] <= lo[0] + O;
    if (counts) {
        t->end.resize((size_t)N);
        for (long j = 0; j < N; ++j) t->end[(size_t)j] = (int32_t)(lo[(size_t)j] - W + K);
        t->H = (int)K - 1;
    }
    return t;
}

}  // namespace

// Periods q < full are complete at g (q O + end[N - 1] <= g); the few behind them (end[N - 1] - end[0] <= O: at most two) are counted
// phase by phase.  q O never leaves 64 bits for g up to 2^62.
long resample_stream_ready(const ResampleHostTable &t, long g) {
    const long O = t.g.O, N = t.g.N, e_min = t.end.front(), e_max = t.end.back();
    const long full = g >= e_max ? (g - e_max) / O + 1 : 0;
    long n = full * N;
    for (long q = full; q * O + e_min <= g; ++q)
        n += std::upper_bound(t.end.begin(), t.end.end(), g - q * O) - t.end.begin();
    return n;
}

std::shared_ptr<const ResampleHostTable> resample_table(int src, int dst) {
    std::lock_guard<std::mutex> g(g_table_mutex);
    auto it = g_tables.find({src, dst});
    if (it != g_tables.end()) return it->second;
    auto t = build_table(src, dst);
    // (a pair that is not served is not remembered: rates arrive from outside -- a snapshot blob names one per record -- and the pairs that
    // ARE served are a bounded set, O and N at most kResampleMaxRatio against two net rates)
    if (t) g_tables[{src, dst}] = t;
    return t;
}

namespace {

// One workgroup = one tile of kResampleTile outputs of one row (see the header of this file).  taps: the transposed image [K][N].
template <typename PcmT>
__global__ void __launch_bounds__(256) resample_rows_kernel(const PcmT *pcm, long ld, const long *lens, const float *taps, const int32_t *first,
                                                            ResampleGeom g, long width_out, float *dst, long ldd, long tiles_per_row) {
    extern __shared__ __align__(16) float span[];
    const long row = blockIdx.x / tiles_per_row, tile = blockIdx.x % tiles_per_row;
    const int t = threadIdx.x;
    const long O = g.O, N = g.N;
    const long m0 = tile * kResampleTile, m1 = m0 + kResampleTile < width_out ? m0 + kResampleTile : width_out;
    long len = lens[row];
    len = len < 0 ? 0 : len > ld ? ld : len;                       // (a row cannot be longer than its pitch: nothing is read past it)
    const long cut = (len * N + O - 1) / O;                          // the row's resampled length
    float *out = dst + row * ldd;
    if (m0 >= cut) {                                                 // the whole tile lies behind the cut
        for (long m = m0 + t; m < m1; m += 256) out[m] = 0.0f;
        return;
    }
    const long mlast = (m1 < cut ? m1 : cut) - 1;
    const long lo = m0 * O / N + g.dlo - g.W;
    const int n_span = (int)(mlast * O / N + g.dhi - g.W + g.K - lo);        // <= g.span (resample_table)
    const PcmT *x = pcm + row * ld;
    for (int s = t; s < n_span; s += 256) {
        const long p = lo + s;
        span[s] = p >= 0 && p < len ? load_pcm(x + p) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kResampleTile / 256; ++i) {
        const long m = m0 + t + 256 * i;
        if (m >= m1) break;
        float acc = 0.0f;
        if (m < cut) {
            const long q = m / N;
            const int j = (int)(m - q * N);
            const float *in = span + (q * O + first[j] - g.W - lo);
            const float *h = taps + j;
            for (int k = 0; k < g.K; ++k) acc = fmaf(h[(long)k * N], in[k], acc);
        }
        out[m] = acc;
    }
}

}  // namespace

hipError_t launch_resample_rows(const ResampleDeviceTable &t, const void *pcm, int esz, long ld, const long *lens, long n, long width_out,
                                float *dst, long ldd, hipStream_t s) {
    if (n <= 0 || width_out <= 0) return hipSuccess;
    const long tiles = (width_out + kResampleTile - 1) / kResampleTile;
    if (tiles * n > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)t.g.span * sizeof(float);
    const dim3 grid((unsigned)(tiles * n)), block(256);
    if (esz == 2)
        hipLaunchKernelGGL(resample_rows_kernel<int16_t>, grid, block, lds, s, static_cast<const int16_t *>(pcm), ld, lens, t.taps, t.first, t.g,
                           width_out, dst, ldd, tiles);
    else
        hipLaunchKernelGGL(resample_rows_kernel<float>, grid, block, lds, s, static_cast<const float *>(pcm), ld, lens, t.taps, t.first, t.g,
                           width_out, dst, ldd, tiles);
    return hipGetLastError();
}

}  // namespace vad

extern "C" {

int vad_resample_geometry(int src, int dst, int *O, int *N, int *W, int *K) {
    auto t = vad::resample_table(src, dst);
    if (!t) return VAD_ERR_SAMPLE_RATE;
    if (O) *O = t->g.O;
    if (N) *N = t->g.N;
    if (W) *W = t->g.W;
    if (K) *K = t->g.K;
    return VAD_OK;
}

long vad_resample_length(int src, int dst, long n) {
    auto t = vad::resample_table(src, dst);
    if (!t) return -VAD_ERR_SAMPLE_RATE;
    if (n < 0) return -VAD_ERR_ARG;
    return (n * t->g.N + t->g.O - 1) / t->g.O;
}

int vad_resample_table(int src, int dst, float *taps, int32_t *first) {
    auto t = vad::resample_table(src, dst);
    if (!t) return VAD_ERR_SAMPLE_RATE;
    if (!taps || !first) return VAD_ERR_ARG;
    std::copy(t->taps.begin(), t->taps.end(), taps);
    std::copy(t->first.begin(), t->first.end(), first);
    return VAD_OK;
}

int vad_resample_host(int src, int dst, const void *pcm, size_t elem_size, long n, float *out) {
    auto t = vad::resample_table(src, dst);
    if (!t) return VAD_ERR_SAMPLE_RATE;
    if ((elem_size != 2 && elem_size != 4) || n < 0 || (n > 0 && (!pcm || !out))) return VAD_ERR_ARG;
    const long O = t->g.O, N = t->g.N, W = t->g.W, K = t->g.K;
    const long n_out = (n * N + O - 1) / O;
    const int16_t *xi = static_cast<const int16_t *>(pcm);
    const float *xf = static_cast<const float *>(pcm);
    for (long m = 0; m < n_out; ++m) {
        const long q = m / N, j = m - q * N;
        const long p0 = q * O + t->first[(size_t)j] - W;
        const float *h = t->taps.data() + j * K;
        double acc = 0.0;
        for (long k = 0; k < K; ++k) {
            const long p = p0 + k;
            if (p < 0 || p >= n) continue;                           // the input is zero outside [0, n)
            acc += (double)h[k] * (elem_size == 2 ? (double)xi[p] / 32768.0 : (double)xf[p]);
        }
        out[m] = (float)acc;
    }
    return VAD_OK;
}

long vad_resample_stream_ready(int src, int dst, long g) {
    auto t = vad::resample_table(src, dst);
    if (!t || t->end.empty()) return -VAD_ERR_SAMPLE_RATE;
    if (g < 0) return -VAD_ERR_ARG;
    return vad::resample_stream_ready(*t, g);
}

int vad_resample_stream_history(int src, int dst) {
    auto t = vad::resample_table(src, dst);
    if (!t || t->end.empty()) return -VAD_ERR_SAMPLE_RATE;
    return t->H;
}

long vad_resample_stream_host(int src, int dst, long g, const int16_t *history, const int16_t *in, long n, float *out, int16_t *history_out) {
    auto t = vad::resample_table(src, dst);
    if (!t || t->end.empty()) return -VAD_ERR_SAMPLE_RATE;
    if (g < 0 || n < 0 || !history || (n > 0 && !in)) return -VAD_ERR_ARG;
    const long O = t->g.O, N = t->g.N, W = t->g.W, K = t->g.K, H = t->H;
    // whole periods that are complete at g leave both counters: the rule is periodic from there on (ready(g + O) = ready(g) + N once
    // g + O >= end[N - 1]), and what is left of g stays below end[N - 1] + O
    const long periods = g >= t->end.back() ? (g - t->end.back()) / O : 0;
    const long g0 = g - periods * O;
    const long m0 = vad::resample_stream_ready(*t, g0), m1 = vad::resample_stream_ready(*t, g0 + n);
    if (m1 > m0 && !out) return -VAD_ERR_ARG;
    for (long m = m0; m < m1; ++m) {
        const long q = m / N, j = m - q * N;
        const long p0 = q * O + t->first[(size_t)j] - W;             // >= g0 - H: the output was not ready at g0
        const float *h = t->taps.data() + j * K;
        double acc = 0.0;
        for (long k = 0; k < K; ++k) {
            const long p = p0 + k;
            const int16_t x = p >= g0 ? in[p - g0] : history[H - (g0 - p)];
            acc += (double)h[k] * ((double)x / 32768.0);
        }
        out[m - m0] = (float)acc;
    }
    if (history_out) {                                               // the last H samples of history ++ in (history_out may be history)
        if (n >= H) std::copy(in + (n - H), in + n, history_out);
        else {
            std::copy(history + n, history + H, history_out);        // (forward, onto lower addresses: safe in place)
            std::copy(in, in + n, history_out + (H - n));
        }
    }
    return m1 - m0;
}

}  // extern "C"
