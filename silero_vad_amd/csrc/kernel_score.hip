// kernel_score.hip -- the validation scores on the device (reference validate(), tuning/utils.py:252-298): per recording the masked BCE
// sums of its chunks, and over the whole corpus the ROC-AUC of every chunk's probability as three integers.  The per-chunk rule and
// the key are scorer.hpp, the source the host twins in segmenter.cpp compile.
//
// score_kernel: one wave per row.  Lane l takes chunks l, l + 64, ... of the row (coalesced), keeps two double sums and three counts,
// writes every chunk's key; the lanes are then folded by a butterfly.  Which chunk goes to which lane depends on the chunk's index
// in the row alone, so a row's sums are the same bits wherever the row lies.
//
// The AUC is a rank statistic over all keys of the corpus, U2 = sum over positives of 2 #{negatives below} + #{negatives equal}.  No
// key carries a payload, so nothing has to be ordered: it is COUNTED.  With v = key >> 1 (31 bits) split into hi = v >> 12 and
// lo = v & 4095:
//   1. auc_hist_kernel     per-class histogram of hi, integer global atomics (2 x 2^19 bins);
//   2. auc_scan_kernel     one workgroup: exclusive scan of the negatives and of the bin sizes, sum of pos[hi] * 2 * neg_below[hi]
//                          -- every pair of a positive and a negative in different bins --, the two class totals;
//   3. auc_scatter_kernel  the keys into bin-contiguous order in the workspace, one atomic cursor per bin, order inside a bin left
//                          to chance;
//   4. auc_bins_kernel     workgroups walk the bins that hold both classes: up to 256 keys are compared all against all from LDS;
//                          more build the two lo histograms in LDS (2 x 4096 x 4 B), scan them and add
//                          pos[lo] * (2 neg_below[lo] + neg[lo]).
// All sums are integers, so the order of the atomics cannot change a result.  Where a whole wave holds one bin (saturated
// probabilities, constant input) its lanes are counted with a ballot and one lane does the atomic.
//
// Known weak spots of the shape: a corpus whose probabilities saturate puts most keys into few bins, so that one workgroup streams a
// long segment while the others are done; and a wave whose keys fall into a few -- but not one -- equal lo values serialises on
// those LDS addresses.
#include <hip/hip_runtime.h>

#include "device_api.hpp"
#include "scorer.hpp"

namespace vad {
namespace {

typedef unsigned long long u64;

constexpr int kLoBits = 12;
constexpr int kLo = 1 << kLoBits;                 // lo values per bin
constexpr int kAucBins = 1 << (31 - kLoBits);     // 2^19 bins of hi: every uint32 key has one
constexpr int kBinThreads = 256;
constexpr int kSmallBin = kBinThreads;            // a bin of at most this many keys is compared all against all
constexpr int kScanThreads = 1024;

__global__ void __launch_bounds__(64) score_kernel(const float *probs, long ldp, const long *row_off, const long *n_chunks,
                                                   const uint8_t *labels, const long *label_off, const long *key_off, uint32_t *keys,
                                                   double *bce_pos, double *bce_neg, int *n_pos, int *n_neg, int *n_bad) {
    const int lane = threadIdx.x;
    const long i = blockIdx.x;
    const long n = n_chunks[i];
    const float *row = probs + (row_off ? row_off[i] : i * ldp);
    const uint8_t *lab = labels + label_off[i];
    uint32_t *out = keys + key_off[i];
    double sp = 0.0, sn = 0.0;
    int cp = 0, cn = 0, cb = 0;
    for (long t = lane; t < n; t += 64) {
        const ScoreChunk c = score_chunk(row[t], lab[t]);
        out[t] = c.key;
        if (c.kind == kScorePos) {
            sp += c.term;
            ++cp;
        } else if (c.kind == kScoreNeg) {
            sn += c.term;
            ++cn;
        } else if (c.kind == kScoreBad) {
            ++cb;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {                        // a + b on both partners: every lane ends with the same bits
        sp += __shfl_xor(sp, m);
        sn += __shfl_xor(sn, m);
        cp += __shfl_xor(cp, m);
        cn += __shfl_xor(cn, m);
        cb += __shfl_xor(cb, m);
    }
    if (lane == 0) {
        bce_pos[i] = sp;
        bce_neg[i] = sn;
        n_pos[i] = cp;
        n_neg[i] = cn;
        n_bad[i] = cb;
    }
}

// ---- the pooled rank statistic -------------------------------------------------------------------------------------------------------
// workspace, uint32 words: neg[kAucBins] | pos[kAucBins] | start[kAucBins] | cursor[kAucBins] | sorted[n]
__device__ inline uint32_t *ws_hist(uint32_t *ws, uint32_t label) { return ws + (size_t)label * kAucBins; }
__device__ inline uint32_t *ws_start(uint32_t *ws) { return ws + 2 * (size_t)kAucBins; }
__device__ inline uint32_t *ws_cursor(uint32_t *ws) { return ws + 3 * (size_t)kAucBins; }
__device__ inline uint32_t *ws_sorted(uint32_t *ws) { return ws + 4 * (size_t)kAucBins; }

// counter[idx] += 1 for every active lane; returns the value the lane's own increment found.  All lanes of the wave call it.  When
// the active lanes share one idx, one lane adds their number and each takes its rank among them.
__device__ inline uint32_t wave_count(uint32_t *counter, bool active, uint32_t idx) {
    const u64 m = __ballot(active);
    if (!m) return 0;
    const int lane = threadIdx.x & 63;
    const int first = __ffsll((long long)m) - 1;
    const uint32_t idx0 = __shfl(idx, first);
    if (__all(!active || idx == idx0)) {
        uint32_t at = 0;
        if (lane == first) at = atomicAdd(counter + idx0, (uint32_t)__popcll(m));
        at = __shfl(at, first);
        return at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    }
    return active ? atomicAdd(counter + idx, 1u) : 0u;
}

__global__ void __launch_bounds__(256) auc_hist_kernel(const uint32_t *keys, long n, uint32_t *ws) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long base = (long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n; base += stride) {     // (base: the same in a wave)
        const long i = base + lane;
        const uint32_t key = i < n ? keys[i] : VAD_SCORE_KEY_NONE;
        // (class and bin in one index: the two histograms lie back to back)
        wave_count(ws, key != VAD_SCORE_KEY_NONE, (key & 1u) * (uint32_t)kAucBins + (key >> (kLoBits + 1)));
    }
}

__device__ inline u64 block_exclusive_scan(u64 x, u64 *wave_tot, u64 *total) {
    // exclusive prefix of x over the workgroup's threads (up to 1 024), the workgroup's sum in *total; two barriers
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, waves = blockDim.x >> 6;
    u64 inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    __syncthreads();                                           // (wave_tot from the previous call has been read)
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
    for (int k = 0; k < waves; ++k) {
        const u64 t = wave_tot[k];
        if (k < w) before += t;
        all += t;
    }
    *total = all;
    return before + inc - x;
}

__global__ void __launch_bounds__(kScanThreads) auc_scan_kernel(uint32_t *ws, u64 *out) {
    __shared__ u64 wave_tot[kScanThreads / 64];
    const uint4 *neg4 = reinterpret_cast<const uint4 *>(ws_hist(ws, 0));
    const uint4 *pos4 = reinterpret_cast<const uint4 *>(ws_hist(ws, 1));
    uint4 *start4 = reinterpret_cast<uint4 *>(ws_start(ws));
    uint4 *cursor4 = reinterpret_cast<uint4 *>(ws_cursor(ws));
    u64 carry = 0;                                             // (keys << 32) | negatives, of the bins in front of the tile: both < 2^31
    u64 u2 = 0;
    for (int g = threadIdx.x; g < kAucBins / 4; g += kScanThreads) {      // kAucBins / 4 is a multiple of the workgroup: no thread leaves early
        const uint4 a = neg4[g], p = pos4[g];
        const uint32_t ng[4] = {a.x, a.y, a.z, a.w}, ps[4] = {p.x, p.y, p.z, p.w};
        u64 mine = 0;
        for (int j = 0; j < 4; ++j) mine += ((u64)(ng[j] + ps[j]) << 32) | ng[j];
        u64 total;
        u64 at = carry + block_exclusive_scan(mine, wave_tot, &total);
        uint32_t st[4];
        for (int j = 0; j < 4; ++j) {
            st[j] = (uint32_t)(at >> 32);
            u2 += (u64)ps[j] * 2ull * (at & 0xFFFFFFFFull);
            at += ((u64)(ng[j] + ps[j]) << 32) | ng[j];
        }
        const uint4 s = make_uint4(st[0], st[1], st[2], st[3]);
        start4[g] = s;
        cursor4[g] = s;
        carry += total;
    }
    u64 total;
    block_exclusive_scan(u2, wave_tot, &total);
    if (threadIdx.x == 0) {
        const u64 n_neg = carry & 0xFFFFFFFFull;
        atomicAdd(out, total);                                 // (out[0] was zeroed in front of this kernel; the bins kernel adds to it)
        out[1] = (carry >> 32) - n_neg;
        out[2] = n_neg;
    }
}

__global__ void __launch_bounds__(256) auc_scatter_kernel(const uint32_t *keys, long n, uint32_t *ws) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * blockDim.x;
    uint32_t *sorted = ws_sorted(ws);
    for (long base = (long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n; base += stride) {
        const long i = base + lane;
        const uint32_t key = i < n ? keys[i] : VAD_SCORE_KEY_NONE;
        const bool active = key != VAD_SCORE_KEY_NONE;
        const uint32_t at = wave_count(ws_cursor(ws), active, key >> (kLoBits + 1));
        if (active && (long)at < n) sorted[at] = key;           // (at < n whenever the keys are those the histogram saw)
    }
}

__global__ void __launch_bounds__(kBinThreads) auc_bins_kernel(uint32_t *ws, long n, u64 *out) {
    __shared__ uint32_t hist[2 * kLo];                         // neg[kLo] | pos[kLo]; a small bin's keys lie in its first words
    __shared__ u64 wave_tot[kBinThreads / 64];
    const uint32_t *neg = ws_hist(ws, 0), *pos = ws_hist(ws, 1), *start = ws_start(ws), *sorted = ws_sorted(ws);
    const int tid = threadIdx.x;
    u64 acc = 0;
    for (int b = blockIdx.x; b < kAucBins; b += gridDim.x) {
        const uint32_t n0 = neg[b], n1 = pos[b];
        if (n0 == 0 || n1 == 0) continue;                      // no pair inside this bin (the same decision in every thread)
        const long m = (long)n0 + n1, s = start[b];
        if (s + m > n) continue;                               // (cannot happen with a consistent workspace: never read past it)
        const uint32_t *seg = sorted + s;
        if (m <= kSmallBin) {
            uint32_t mine = 0;
            if (tid < m) hist[tid] = mine = seg[tid];
            __syncthreads();
            if (tid < m && (mine & 1u)) {
                const uint32_t v = mine >> 1;
                uint32_t c = 0;
                for (int j = 0; j < (int)m; ++j) {
                    const uint32_t o = hist[j];                // (a broadcast)
                    if (!(o & 1u)) c += ((o >> 1) < v ? 2u : 0u) + ((o >> 1) == v ? 1u : 0u);
                }
                acc += c;
            }
            __syncthreads();
            continue;
        }
        for (int k = tid; k < 2 * kLo; k += kBinThreads) hist[k] = 0;
        __syncthreads();
        for (long base = 0; base < m; base += 4 * kBinThreads) {      // (base: the same in the workgroup; four loads in flight a thread)
            uint32_t key[4];
            bool in[4];
            for (int j = 0; j < 4; ++j) {
                const long k = base + j * kBinThreads + tid;
                in[j] = k < m;
                key[j] = in[j] ? seg[k] : 0u;
            }
            for (int j = 0; j < 4; ++j) wave_count(hist, in[j], (key[j] & 1u) * (uint32_t)kLo + ((key[j] >> 1) & (uint32_t)(kLo - 1)));
        }
        __syncthreads();
        constexpr int per = kLo / kBinThreads;                 // consecutive lo values per thread
        uint32_t below = 0;
        for (int j = 0; j < per; ++j) below += hist[tid * per + j];
        u64 total;
        u64 at = block_exclusive_scan(below, wave_tot, &total);
        for (int j = 0; j < per; ++j) {
            const uint32_t a = hist[tid * per + j], p = hist[kLo + tid * per + j];
            acc += (u64)p * (2ull * at + a);
            at += a;
        }
        __syncthreads();                                       // the next bin zeroes what the slowest thread may still read
    }
    u64 total;
    block_exclusive_scan(acc, wave_tot, &total);
    if (tid == 0 && total) atomicAdd(out, total);
}

}  // namespace

hipError_t launch_chunk_scores(const float *probs, long ldp, const long *row_off, long n_rows, const long *n_chunks, const uint8_t *labels,
                               const long *label_off, const long *key_off, uint32_t *keys, double *bce_pos, double *bce_neg, int *n_pos,
                               int *n_neg, int *n_bad, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)n_rows), dim3(64), 0, s, probs, ldp, row_off, n_chunks, labels, label_off, key_off, keys,
                       bce_pos, bce_neg, n_pos, n_neg, n_bad);
    return hipGetLastError();
}

size_t auc_workspace_bytes(long n) { return 4 * (4 * (size_t)kAucBins + (size_t)n); }

hipError_t launch_auc_counts(const uint32_t *keys, long n, void *workspace, unsigned long long *out, hipStream_t s) {
    hipError_t rc = hipMemsetAsync(out, 0, 3 * sizeof(u64), s);
    if (rc != hipSuccess || n <= 0) return rc;
    uint32_t *ws = static_cast<uint32_t *>(workspace);
    rc = hipMemsetAsync(ws, 0, 2 * (size_t)kAucBins * sizeof(uint32_t), s);      // the two histograms; start and cursor are written by the scan
    if (rc != hipSuccess) return rc;
    const unsigned stream_blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(auc_hist_kernel, dim3(stream_blocks), dim3(256), 0, s, keys, n, ws);
    hipLaunchKernelGGL(auc_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ws, out);
    hipLaunchKernelGGL(auc_scatter_kernel, dim3(stream_blocks), dim3(256), 0, s, keys, n, ws);
    hipLaunchKernelGGL(auc_bins_kernel, dim3(2048), dim3(kBinThreads), 0, s, ws, n, out);
    return hipGetLastError();
}

}  // namespace vad
