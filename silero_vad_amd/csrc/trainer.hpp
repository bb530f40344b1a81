// trainer.hpp -- the decoder's training rule (reference train(), tuning/utils.py:206-249, over VADDecoderRNNJIT): what one chunk
// contributes to the masked BCE loss and what the head hands back to the recurrence.  Written once for the host twin (trainer.cpp,
// vad_decoder_grad_host, everything in double) and for the device (kernel_train.hip, fp32 with the log in double).
//
// Row b runs from zero (h, c) over t < n_chunks[b]; nothing behind that is read.  Per step, aten::lstm_cell in gate order i, f, g, o:
//   G = W_ih feat_t + b_ih + W_hh h_{t-1} + b_hh,  i, f, o = sigmoid, g = tanh,  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
//   y = keep ? relu(h_t) keep_scale : 0   (keep == NULL: y = relu(h_t)),   z = w_out y + b_out,   p = sigmoid(z)
// Chunk weight w: 1 for label 1, noise_loss for label 0, 0 for any other label (255 = VAD_LABEL_IGNORE: a chunk that is not there).
//   loss = sum w bce(p, label) / denom,  bce = nn.BCELoss's term with its -100 clamp, the log in double (scorer.hpp)
// The head's backward is the reference's two steps (BCELoss backward with eps 1e-12, then sigmoid backward) in one expression on the
// FLOAT32 probability:
//   dz = (w / denom) (p - label) [p (1 - p) / max(p (1 - p), 1e-12)]
// so that a chunk whose fp32 p is exactly 0 or 1 hands back nothing, as under torch.  The rest is plain BPTT:
//   dh_t = keep_scale keep [h_t > 0] w_out dz_t + W_hh^T dG_{t+1},   do = dh tanh(c),   dc_t = dh o (1 - tanh(c)^2) + f_{t+1} dc_{t+1}
//   dG_i = dc g i (1 - i),  dG_f = dc c_{t-1} f (1 - f),  dG_g = dc i (1 - g^2),  dG_o = do o (1 - o)
//   dW_ih = sum dG_t^T feat_t,  dW_hh = sum dG_t^T h_{t-1},  db_ih = db_hh = sum dG_t,  dw_out = sum dz y,  db_out = sum dz
//
// Workspace of the device call (vad_decoder_grad_workspace_bytes), N = B T chunks, S = train_splits(N) split-K slabs:
//   GX[N][512] | dG[N][512] | stash[N][7][128] (i, f, g, o, c, tanh c, h) | dz[N]   float32
//   flags[N] uint8 | row_loss[B] double | slabs[S][2 * 512 * 128 + 512 + 128 + 1] float32
// each part rounded up to 256 bytes: about N (512 * 2 + 7 * 128) * 4 bytes plus at most 34 MB of slabs (280 MB in all at 128 x 250).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VAD_TRAIN_HD __host__ __device__
#else
#define VAD_TRAIN_HD
#endif

namespace vad {

constexpr int kTrainH = 128;                       // hidden units = encoder features
constexpr int kTrainG = 4 * kTrainH;               // gate rows
constexpr int kTrainStash = 7 * kTrainH;           // floats the forward keeps per chunk
constexpr long kTrainMaxSplits = 64;               // split-K slabs of the reductions over B T
constexpr long kTrainMinSplit = 256;               // ... of at least this many chunks each
constexpr size_t kTrainSlabFloats = 2 * (size_t)kTrainG * kTrainH + kTrainG + kTrainH + 1;   // dW_ih | dW_hh | db | dw_out | db_out

// chunks per slab (a multiple of 4, the MFMA's K) and the number of slabs
VAD_TRAIN_HD inline long train_split_len(long n) {
    long len = (n + kTrainMaxSplits - 1) / kTrainMaxSplits;
    if (len < kTrainMinSplit) len = kTrainMinSplit;
    return (len + 3) / 4 * 4;
}
VAD_TRAIN_HD inline long train_splits(long n) {
    const long len = train_split_len(n);
    return (n + len - 1) / len;
}

struct TrainLayout {
    size_t gx, dg, stash, dz, flags, row_loss, slabs, total;     // byte offsets
};
VAD_TRAIN_HD inline size_t train_up(size_t x) { return (x + 255) / 256 * 256; }
VAD_TRAIN_HD inline TrainLayout train_layout(int B, long T) {
    const size_t n = (size_t)B * (size_t)T;
    TrainLayout l{};
    size_t at = 0;
    l.gx = at;       at += train_up(n * kTrainG * 4);
    l.dg = at;       at += train_up(n * kTrainG * 4);
    l.stash = at;    at += train_up(n * kTrainStash * 4);
    l.dz = at;       at += train_up(n * 4);
    l.flags = at;    at += train_up(n);
    l.row_loss = at; at += train_up((size_t)B * 8);
    l.slabs = at;    at += train_up((size_t)train_splits((long)n) * kTrainSlabFloats * 4);
    l.total = at;
    return l;
}

VAD_TRAIN_HD inline double train_weight(unsigned label, double noise_loss) { return label == 1u ? 1.0 : label == 0u ? noise_loss : 0.0; }

// BCELoss's term of one chunk on the fp32 probability (label 0 / 1 only); a NaN probability gives NaN
VAD_TRAIN_HD inline double train_bce(float p, unsigned label) {
    const float q = label ? p : 1.0f - p;
    const double l = log((double)q);
    return 0.0 - (l < -100.0 ? -100.0 : l);
}

// d loss / d z of one chunk, on the fp32 probability
VAD_TRAIN_HD inline double train_dz(float p, unsigned label, double w, double denom) {
    if (w == 0.0) return 0.0;
    const double pd = (double)p, pq = pd * (1.0 - pd);
    return (w / denom) * (pd - (double)label) * (pq / (pq > 1e-12 ? pq : 1e-12));
}

}  // namespace vad
