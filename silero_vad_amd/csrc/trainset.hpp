// trainset.hpp -- the rules of resident training: how a batch row is cut out of a corpus that lies in one arena (the reference's
// SileroVadDataset.__getitem__ + collate, tuning/utils.py:84-160, without the random crop), and torch.optim.Adam's update of one
// parameter.  Written once for the host twins (trainset.cpp: vad_trainset_batch_host, vad_decoder_adam_host in double) and for the
// device (kernel_trainset.hip: the same row rule, the update in float32).
//
// Row b of a batch takes recording r = idx[b] of N:
//   len = min(lens[r], max_samples) (0 for r outside [0, N) or lens[r] < 0),  n_chunks = ceil(len / chunk)
//   pcm[b][0 .. len) = arena[offs[r] ..) in the arena's element type, exact zeros from len to the pitch
//   labels[b][t] = label_arena[label_offs[r] + t] for t < n_chunks, VAD_LABEL_IGNORE (255) from there to the pitch
// Adam (no amsgrad, no weight decay, not maximize), step t >= 1, the bias corrections taken on the host in double:
//   m = m + (g - m)(1 - beta1),  v = beta2 v + (1 - beta2) g g,  p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// in the order of torch's composed operations (lerp_, mul_ + addcmul_, sqrt / div / add_, addcdiv_).  Step 1 starts the state: m and v
// count as zero whatever they hold.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VAD_TRAINSET_HD __host__ __device__
#else
#define VAD_TRAINSET_HD
#endif

namespace vad {

constexpr int kAdamTensors = 6;
// w_ih, w_hh, b_ih, b_hh, w_out, b_out: the fields of vad_decoder_params in order; 132 225 parameters
constexpr long kAdamCounts[kAdamTensors] = {512 * 128, 512 * 128, 512, 512, 128, 1};
constexpr long kAdamTotal = 2 * 512 * 128 + 2 * 512 + 128 + 1;

struct TrainRow {
    long len, n_chunks;
};

// recording r of n_recordings cut for a batch row; chunk > 0, max_samples >= 0
VAD_TRAINSET_HD inline TrainRow trainset_row(const long *lens, long n_recordings, long r, long max_samples, long chunk) {
    long len = (r >= 0 && r < n_recordings) ? lens[r] : 0;
    if (len < 0) len = 0;
    if (len > max_samples) len = max_samples;
    return TrainRow{len, (len + chunk - 1) / chunk};
}

// what Adam's step needs besides the state: every factor in the precision of the update (float on the device, double in the twin)
template <typename T>
struct AdamFactors {
    T one_minus_beta1, beta2, one_minus_beta2, step_size, bias2_sqrt, eps;
};

template <typename T>
inline AdamFactors<T> adam_factors(long step, double lr, double beta1, double beta2, double eps) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    return AdamFactors<T>{(T)(1.0 - beta1), (T)beta2, (T)(1.0 - beta2), (T)(lr / bc1), (T)std::sqrt(bc2), (T)eps};
}

// One parameter's step; a non-finite gradient propagates as under torch.  Each line is one of torch's composed operations with the
// roundings its CPU kernels make -- lerp_ is one fused multiply-add, mul_ / addcmul_ and sqrt / div / add_ / addcdiv_ round after every
// operation -- so nothing here may be contracted further: in float32 this is torch's arithmetic, not merely its formula.
template <typename T>
VAD_TRAINSET_HD inline void adam_update(T &p, T &m, T &v, T g, const AdamFactors<T> &f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
    using std::fma;
    using std::sqrt;
#endif
    m = fma(f.one_minus_beta1, g - m, m);                          // exp_avg.lerp_(grad, 1 - beta1)
    v = v * f.beta2;                                               // exp_avg_sq.mul_(beta2)
    v = v + (f.one_minus_beta2 * g) * g;                           //           .addcmul_(grad, grad, value = 1 - beta2)
    const T denom = sqrt(v) / f.bias2_sqrt + f.eps;                // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p + ((T)0 - f.step_size) * m / denom;                      // param.addcdiv_(exp_avg, denom, value = -step_size)
}

}  // namespace vad
