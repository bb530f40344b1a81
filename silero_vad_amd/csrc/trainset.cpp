// trainset.cpp -- the host twins of resident training (the rules: trainset.hpp): vad_trainset_batch_host cuts a padded batch out of
// an arena in host memory, vad_decoder_adam_host is torch.optim.Adam's step in double.  Pure C++, what the device calls are tested
// against.
#include <cstring>
#include <vector>

#include "../../include/silero_vad_hip.h"
#include "trainset.hpp"

extern "C" int vad_trainset_batch_host(const void *arena, size_t elem_size, const long *offs, const long *lens, const uint8_t *label_arena,
                                       const long *label_offs, long n_recordings, const long *idx, long B, long max_samples, long chunk,
                                       void *out_pcm, long ld, uint8_t *out_labels, long ldl, long *out_lens, long *out_n_chunks) {
    if (!arena || !offs || !lens || !label_arena || !label_offs || !idx || !out_pcm || !out_labels || !out_lens || !out_n_chunks) return VAD_ERR_ARG;
    if ((elem_size != 2 && elem_size != 4) || n_recordings <= 0 || B <= 0 || chunk <= 0 || ld <= 0 || ldl <= 0 || max_samples < 0) return VAD_ERR_ARG;
    // every row is checked before the first byte is written
    std::vector<vad::TrainRow> rows((size_t)B);
    for (long b = 0; b < B; ++b) {
        const long r = idx[b];
        if (r < 0 || r >= n_recordings || lens[r] < 0) return VAD_ERR_ARG;
        rows[b] = vad::trainset_row(lens, n_recordings, r, max_samples, chunk);
        if (rows[b].len > ld || rows[b].n_chunks > ldl) return VAD_ERR_ARG;
    }
    const char *src = static_cast<const char *>(arena);
    char *dst = static_cast<char *>(out_pcm);
    for (long b = 0; b < B; ++b) {
        const long r = idx[b], len = rows[b].len, nck = rows[b].n_chunks;
        char *row = dst + (size_t)b * ld * elem_size;
        if (len) std::memcpy(row, src + (size_t)offs[r] * elem_size, (size_t)len * elem_size);
        std::memset(row + (size_t)len * elem_size, 0, (size_t)(ld - len) * elem_size);
        uint8_t *lab = out_labels + (size_t)b * ldl;
        if (nck) std::memcpy(lab, label_arena + label_offs[r], (size_t)nck);
        std::memset(lab + nck, VAD_LABEL_IGNORE, (size_t)(ldl - nck));
        out_lens[b] = len;
        out_n_chunks[b] = nck;
    }
    return VAD_OK;
}

extern "C" int vad_decoder_adam_host(const vad_decoder_grads_f64 *params, const vad_decoder_params_f64 *grads, const vad_decoder_grads_f64 *m,
                                     const vad_decoder_grads_f64 *v, long step, double lr, double beta1, double beta2, double eps) {
    if (!params || !grads || !m || !v || step < 1) return VAD_ERR_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(lr >= 0.0) || !(eps >= 0.0)) return VAD_ERR_ARG;
    double *const pp[] = {params->w_ih, params->w_hh, params->b_ih, params->b_hh, params->w_out, params->b_out};
    const double *const gg[] = {grads->w_ih, grads->w_hh, grads->b_ih, grads->b_hh, grads->w_out, grads->b_out};
    double *const mm[] = {m->w_ih, m->w_hh, m->b_ih, m->b_hh, m->w_out, m->b_out};
    double *const vv[] = {v->w_ih, v->w_hh, v->b_ih, v->b_hh, v->w_out, v->b_out};
    for (int k = 0; k < vad::kAdamTensors; ++k)
        if (!pp[k] || !gg[k] || !mm[k] || !vv[k] || ((size_t)pp[k] & 7) || ((size_t)gg[k] & 7) || ((size_t)mm[k] & 7) || ((size_t)vv[k] & 7))
            return VAD_ERR_ARG;
    const vad::AdamFactors<double> f = vad::adam_factors<double>(step, lr, beta1, beta2, eps);
    for (int k = 0; k < vad::kAdamTensors; ++k)
        for (long i = 0; i < vad::kAdamCounts[k]; ++i) {
            if (step == 1) mm[k][i] = vv[k][i] = 0.0;             // step 1 starts the state
            vad::adam_update<double>(pp[k][i], mm[k][i], vv[k][i], gg[k][i], f);
        }
    return VAD_OK;
}
