// kernel_sweep.hip -- the enter / exit threshold sweep on the device: for every row of probabilities and every (enter, exit) pair the
// confusion counts of the hysteresis decision against per-chunk labels (reference: the loops of calculate_best_thresholds,
// tuning/utils.py:326-356; the decision and the counts are sweeper.hpp, the same source the host twin in segmenter.cpp compiles).
//
// Why on the device: the probabilities already sit in HBM when a bucket's kernels finish.  The reference walks every chunk once per
// pair in Python (190 pairs on its 20 x 20 grid); bringing the probabilities home to do the same on the host costs 4 B per chunk
// over the link.  Here only the integer counts come back, 2 x 4 B per (row, pair).
//
// Shape: one wave per (row, block of 64 pairs).  The decision is carried from chunk to chunk, so a row is never split along time;
// the parallel axes are the row and the pair.  A lane keeps its pair's thresholds, decision and two counts in registers.  The row is
// walked in tiles of kSweepTile chunks: the wave copies the tile's probabilities and labels into LDS (16-byte loads where the
// granule lies inside the row, element by element at the row's two ends), then every lane reads the SAME LDS address chunk after
// chunk -- a broadcast, no bank conflicts -- and feeds its own cell.
//
// Tiles are cut on the 16-byte grid of the probabilities' ADDRESS, not of the row: with s = the row start's offset inside its
// granule (0 ... 3 floats), chunk t sits at grid position u = s + t, and tile k holds u in [k * kSweepTile, (k + 1) * kSweepTile).
// Every full granule is then an aligned float4 in HBM and in LDS alike.  Grid positions outside the row (the up to three in front of
// its first chunk, everything behind its last) are never loaded: their LDS labels are VAD_LABEL_IGNORE, which the cell skips, so
// the inner loop runs over whole granules without a bounds test and whatever the batch holds around the live chunks cannot matter.
#include <hip/hip_runtime.h>

#include "device_api.hpp"
#include "sweeper.hpp"

namespace vad {
namespace {

constexpr int kSweepTile = 1024;             // chunks per tile: 4 KiB of probabilities + 1 KiB of labels in LDS
constexpr int kSweepGran = kSweepTile / 4;

__global__ void __launch_bounds__(64) sweep_kernel(const float *probs, long ldp, const long *row_off, const long *n_chunks,
                                                   const uint8_t *labels, const long *label_off, const float *enter, const float *exit_,
                                                   int n_pairs, int pair_blocks, int *tp, int *tn, int *n_pos, int *n_valid) {
    __shared__ float4 sp[kSweepGran];
    __shared__ uint32_t sl[kSweepGran];
    const int lane = threadIdx.x;
    const long i = blockIdx.x / pair_blocks;
    const int pb = blockIdx.x % pair_blocks;
    const int k = pb * 64 + lane;
    const bool live = k < n_pairs;
    const float en = live ? enter[k] : 0.f, ex = live ? exit_[k] : 0.f;

    const long n = n_chunks[i];
    const float *row = probs + (row_off ? row_off[i] : i * ldp);
    const uint8_t *lab = labels + label_off[i];
    const long s = (long)((((size_t)row) >> 2) & 3);         // the row start inside its 16-byte granule, in floats
    const float *grid = row - s;                              // 16-byte aligned; grid[u] is chunk u - s
    const long end = s + n;                                   // grid positions [s, end) are the row

    SweepCell cell;
    SweepLabels seen;
    for (long base = 0; base < end; base += kSweepTile) {
        const long left = end - base;
        const int grans = (int)((left < kSweepTile ? left : kSweepTile) + 3) / 4;
        for (int g = lane; g < grans; g += 64) {
            const long u = base + 4 * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t w;
            if (u >= s && u + 4 <= end) {
                v = *reinterpret_cast<const float4 *>(grid + u);
                const uint8_t *l = lab + (u - s);
                w = (uint32_t)l[0] | ((uint32_t)l[1] << 8) | ((uint32_t)l[2] << 16) | ((uint32_t)l[3] << 24);
            } else {                                          // a granule at one of the row's ends: only what lies inside the row
                float e[4] = {0.f, 0.f, 0.f, 0.f};
                w = 0;
                for (int j = 0; j < 4; ++j) {
                    const bool in = u + j >= s && u + j < end;
                    if (in) e[j] = grid[u + j];
                    w |= (uint32_t)(in ? lab[u + j - s] : (uint8_t)VAD_LABEL_IGNORE) << (8 * j);
                }
                v = make_float4(e[0], e[1], e[2], e[3]);
            }
            sp[g] = v;
            sl[g] = w;
        }
        __syncthreads();
        for (int g = 0; g < grans; ++g) {
            const float4 v = sp[g];
            const uint32_t w = sl[g];
            cell.feed(v.x, w & 255u, en, ex);
            cell.feed(v.y, (w >> 8) & 255u, en, ex);
            cell.feed(v.z, (w >> 16) & 255u, en, ex);
            cell.feed(v.w, w >> 24, en, ex);
            seen.feed(w & 255u);
            seen.feed((w >> 8) & 255u);
            seen.feed((w >> 16) & 255u);
            seen.feed(w >> 24);
        }
        __syncthreads();                                      // the next tile overwrites what the slowest lane may still read
    }
    if (live) {
        tp[i * n_pairs + k] = cell.tp;
        tn[i * n_pairs + k] = cell.tn;
    }
    if (pb == 0 && lane == 0) {
        n_pos[i] = seen.n_pos;
        n_valid[i] = seen.n_valid;
    }
}

}  // namespace

hipError_t launch_sweep(const float *probs, long ldp, const long *row_off, long n_rows, const long *n_chunks, const uint8_t *labels,
                        const long *label_off, const float *enter, const float *exit_, long n_pairs, int *tp, int *tn, int *n_pos,
                        int *n_valid, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const long pair_blocks = (n_pairs + 63) / 64;
    hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)(n_rows * pair_blocks)), dim3(64), 0, s, probs, ldp, row_off, n_chunks, labels, label_off,
                       enter, exit_, (int)n_pairs, (int)pair_blocks, tp, tn, n_pos, n_valid);
    return hipGetLastError();
}

}  // namespace vad
