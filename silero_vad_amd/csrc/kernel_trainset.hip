// kernel_trainset.hip -- resident training: a padded batch cut out of a corpus that already lies in HBM, and torch.optim.Adam's step
// over the six decoder tensors in one launch (the rules: trainset.hpp).
//
//   trainset_batch_kernel    workgroup (b, j) writes 256 x 16 bytes of row b of the batch: a 16-byte vector a thread, loaded as one
//                            vector where the recording's address is 16-byte aligned and the vector lies inside the cut, element by
//                            element otherwise (a recording at an odd sample of the arena, the vector that straddles the cut's end) --
//                            the same bytes either way -- and exact zeros behind the cut, to the pitch.  Workgroup (b, 0) also writes
//                            the row's labels over their pitch, its length and its chunk count.
//   train_adam_reset_kernel  m = v = 0: queued in front of step 1 only, never again, so a later step cannot zero live state.
//   train_adam_kernel        thread i owns parameter i of the 132 225; the bias corrections arrive as arguments, there is no counter
//                            on the device.
// The source is HBM, not the host link: the grid is as wide as the batch (kernel_ingest.hip's 96 waves exist to spare PCIe ingest's
// neighbours; a batch of 128 x 8 s is 32 MB and leaves in microseconds).  No atomics; a row's bytes depend on its recording alone.
#include <hip/hip_runtime.h>

#include "device_api.hpp"
#include "trainset.hpp"

namespace vad {
namespace {

constexpr int kBatchThreads = 256;

template <typename E>
__global__ void __launch_bounds__(kBatchThreads) trainset_batch_kernel(const E *arena, const long *offs, const long *lens, const uint8_t *label_arena,
                                                                       const long *label_offs, long n_recordings, const long *idx,
                                                                       long max_samples, long chunk, E *out_pcm, long ld, int vec_out,
                                                                       uint8_t *out_labels, long ldl, long *out_lens, long *out_n_chunks,
                                                                       long blocks_per_row) {
    using u32x4 = unsigned __attribute__((ext_vector_type(4)));
    constexpr int V = 16 / (int)sizeof(E);                      // elements of one 16-byte vector
    const long b = blockIdx.x / blocks_per_row, j = blockIdx.x % blocks_per_row;
    const long r = idx[b];
    // the call cannot see lens on the host: a cut longer than the pitches is cut again at the pitches, never written past them
    const TrainRow row = trainset_row(lens, n_recordings, r, max_samples < ld ? max_samples : ld, chunk);
    const long len = row.len;
    const E *src = len > 0 ? arena + offs[r] : arena;
    E *dst = out_pcm + b * ld;
    const long e0 = (j * kBatchThreads + threadIdx.x) * (long)V;
    if (e0 < ld) {
        union {
            u32x4 q;
            E e[V];
        } u;
        u.q = u32x4{0u, 0u, 0u, 0u};
        if (e0 + V <= len && (((size_t)(src + e0)) & 15) == 0) {
            u.q = *reinterpret_cast<const u32x4 *>(src + e0);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (e0 + k < len) u.e[k] = src[e0 + k];
        }
        if (vec_out) {                                          // the pitch and the base are 16-byte multiples: e0 + V <= ld
            *reinterpret_cast<u32x4 *>(dst + e0) = u.q;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (e0 + k < ld) dst[e0 + k] = u.e[k];
        }
    }
    if (j == 0) {
        const long nck = row.n_chunks < ldl ? row.n_chunks : ldl;
        const uint8_t *ls = nck > 0 ? label_arena + label_offs[r] : label_arena;
        for (long t = threadIdx.x; t < ldl; t += kBatchThreads) out_labels[b * ldl + t] = t < nck ? ls[t] : (uint8_t)VAD_LABEL_IGNORE;
        if (threadIdx.x == 0) {
            out_lens[b] = len;
            out_n_chunks[b] = nck;
        }
    }
}

struct AdamPtrs {
    float *p[kAdamTensors];
    const float *g[kAdamTensors];
    float *m[kAdamTensors], *v[kAdamTensors];
};

// parameter i of the 132 225 -> (tensor, element)
__device__ inline int adam_locate(long &i) {
    int k = 0;
#pragma unroll
    for (int q = 0; q < kAdamTensors - 1; ++q)
        if (k == q && i >= kAdamCounts[q]) {
            i -= kAdamCounts[q];
            k = q + 1;
        }
    return k;
}

__global__ void __launch_bounds__(256) train_adam_reset_kernel(AdamPtrs a) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kAdamTotal) return;
    const int k = adam_locate(i);
    a.m[k][i] = 0.0f;
    a.v[k][i] = 0.0f;
}

__global__ void __launch_bounds__(256) train_adam_kernel(AdamPtrs a, AdamFactors<float> f) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kAdamTotal) return;
    const int k = adam_locate(i);
    float p = a.p[k][i], m = a.m[k][i], v = a.v[k][i];
    adam_update<float>(p, m, v, a.g[k][i], f);
    a.p[k][i] = p;
    a.m[k][i] = m;
    a.v[k][i] = v;
}

}  // namespace

hipError_t launch_trainset_batch(const TrainsetArgs &a, hipStream_t s) {
    const long V = 16 / a.elem_size;
    const long blocks_per_row = (a.ld + V * kBatchThreads - 1) / (V * kBatchThreads);
    const unsigned grid = (unsigned)(blocks_per_row * a.B);
    const int vec_out = (((size_t)a.out_pcm & 15) == 0 && (a.ld * a.elem_size) % 16 == 0) ? 1 : 0;
    if (a.elem_size == 2)
        hipLaunchKernelGGL(trainset_batch_kernel<int16_t>, dim3(grid), dim3(kBatchThreads), 0, s, static_cast<const int16_t *>(a.arena), a.offs, a.lens,
                           a.label_arena, a.label_offs, a.n_recordings, a.idx, a.max_samples, a.chunk, static_cast<int16_t *>(a.out_pcm), a.ld,
                           vec_out, a.out_labels, a.ldl, a.out_lens, a.out_n_chunks, blocks_per_row);
    else
        hipLaunchKernelGGL(trainset_batch_kernel<float>, dim3(grid), dim3(kBatchThreads), 0, s, static_cast<const float *>(a.arena), a.offs, a.lens,
                           a.label_arena, a.label_offs, a.n_recordings, a.idx, a.max_samples, a.chunk, static_cast<float *>(a.out_pcm), a.ld,
                           vec_out, a.out_labels, a.ldl, a.out_lens, a.out_n_chunks, blocks_per_row);
    return hipGetLastError();
}

hipError_t launch_decoder_adam(const vad_decoder_grads &p, const vad_decoder_params &g, const vad_decoder_grads &m, const vad_decoder_grads &v,
                               long step, double lr, double beta1, double beta2, double eps, hipStream_t s) {
    AdamPtrs a;
    float *const pp[] = {p.w_ih, p.w_hh, p.b_ih, p.b_hh, p.w_out, p.b_out};
    const float *const gg[] = {g.w_ih, g.w_hh, g.b_ih, g.b_hh, g.w_out, g.b_out};
    float *const mm[] = {m.w_ih, m.w_hh, m.b_ih, m.b_hh, m.w_out, m.b_out};
    float *const vv[] = {v.w_ih, v.w_hh, v.b_ih, v.b_hh, v.w_out, v.b_out};
    for (int k = 0; k < kAdamTensors; ++k) {
        a.p[k] = pp[k];
        a.g[k] = gg[k];
        a.m[k] = mm[k];
        a.v[k] = vv[k];
    }
    const unsigned grid = (unsigned)((kAdamTotal + 255) / 256);
    if (step == 1) hipLaunchKernelGGL(train_adam_reset_kernel, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(train_adam_kernel, dim3(grid), dim3(256), 0, s, a, adam_factors<float>(step, lr, beta1, beta2, eps));
    return hipGetLastError();
}

}  // namespace vad
