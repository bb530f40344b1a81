// trainer.cpp -- vad_decoder_grad_host: the rule of trainer.hpp in double, the reference the device call is tested against.  Pure C++.
//
// Phase 1, rows in parallel: forward with every activation kept, backward to dG[n][512].  Phase 2, gate rows in parallel: the sums
// over n = b T + t in ascending n.  Each number is produced by one thread in a fixed order, so the result does not depend on
// `threads`.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/silero_vad_hip.h"
#include "host_threads.hpp"
#include "trainer.hpp"

namespace {

constexpr int H = vad::kTrainH, G = vad::kTrainG;

template <typename F>
void run_parallel(long n, int threads, F fn) {
    const int nt = (int)std::max<long>(1, std::min<long>(threads, n));
    if (nt == 1) {
        for (long i = 0; i < n; ++i) fn(i);
        return;
    }
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w)
        pool.emplace_back([=] {
            for (long i = w; i < n; i += nt) fn(i);
        });
    for (auto &t : pool) t.join();
}

inline double sigmoid_d(double x) { return 1.0 / (1.0 + std::exp(-x)); }

struct Step {
    double a[G];       // activated gates i, f, g, o
    double c[H], tc[H], h[H], y[H];
    double dz;
};

}  // namespace

extern "C" int vad_decoder_grad_host(const vad_decoder_params_f64 *p, const float *feat, int B, long T, const long *n_chunks,
                                     const uint8_t *labels, long ldl, const uint8_t *keep, float keep_scale, float noise_loss, double denom,
                                     vad_decoder_grads_f64 *g, double *loss, float *probs, int threads) {
    if (!p || !g || !feat || !n_chunks || !labels || !loss || B <= 0 || T <= 0 || ldl < T || !(denom > 0.0)) return VAD_ERR_ARG;
    if (!p->w_ih || !p->w_hh || !p->b_ih || !p->b_hh || !p->w_out || !p->b_out) return VAD_ERR_ARG;
    if (!g->w_ih || !g->w_hh || !g->b_ih || !g->b_hh || !g->w_out || !g->b_out) return VAD_ERR_ARG;
    const void *dbl[] = {p->w_ih, p->w_hh, p->b_ih, p->b_hh, p->w_out, p->b_out, g->w_ih, g->w_hh, g->b_ih, g->b_hh, g->w_out, g->b_out, loss};
    for (const void *q : dbl)
        if ((size_t)q & 7) return VAD_ERR_ARG;
    if (((size_t)feat & 3) || ((size_t)probs & 3) || ((size_t)n_chunks & 7)) return VAD_ERR_ARG;
    for (int b = 0; b < B; ++b)
        if (n_chunks[b] < 0 || n_chunks[b] > T) return VAD_ERR_ARG;
    const int nt = threads > 0 ? threads : vad::default_host_threads(64);
    const size_t N = (size_t)B * (size_t)T;
    std::vector<double> dG(N * G, 0.0), hs(N * H, 0.0), ys(N * H, 0.0), dzs(N, 0.0), row_loss((size_t)B, 0.0);
    const double ks = keep ? (double)keep_scale : 1.0, nl = (double)noise_loss;

    run_parallel(B, nt, [&](long b) {
        const long nc = n_chunks[b];
        if (nc == 0) return;
        std::vector<Step> st((size_t)nc);
        std::vector<double> h(H, 0.0), c(H, 0.0), pre(G);
        double ls = 0.0;
        for (long t = 0; t < nc; ++t) {
            const size_t n = (size_t)b * T + t;
            const float *x = feat + n * H;
            Step &s = st[t];
            for (int j = 0; j < G; ++j) {
                double a = p->b_ih[j] + p->b_hh[j];
                const double *wi = p->w_ih + (size_t)j * H, *wh = p->w_hh + (size_t)j * H;
                for (int k = 0; k < H; ++k) a += wi[k] * (double)x[k];
                for (int k = 0; k < H; ++k) a += wh[k] * h[k];
                pre[j] = a;
            }
            double z = p->b_out[0];
            for (int k = 0; k < H; ++k) {
                s.a[k] = sigmoid_d(pre[k]);
                s.a[H + k] = sigmoid_d(pre[H + k]);
                s.a[2 * H + k] = std::tanh(pre[2 * H + k]);
                s.a[3 * H + k] = sigmoid_d(pre[3 * H + k]);
                c[k] = s.a[H + k] * c[k] + s.a[k] * s.a[2 * H + k];
                s.c[k] = c[k];
                s.tc[k] = std::tanh(c[k]);
                h[k] = s.a[3 * H + k] * s.tc[k];
                s.h[k] = h[k];
                const double r = h[k] <= 0.0 ? (h[k] != h[k] ? h[k] : 0.0) : h[k];     // relu that keeps NaN
                s.y[k] = keep ? (keep[n * H + k] ? r * ks : 0.0) : r;
                z += p->w_out[k] * s.y[k];
                hs[n * H + k] = h[k];
                ys[n * H + k] = s.y[k];
            }
            const float pf = (float)sigmoid_d(z);                 // the head's probability as the reference holds it
            if (probs) probs[n] = pf;
            const unsigned lab = labels[(size_t)b * ldl + t];
            const double w = vad::train_weight(lab, nl);
            if (w != 0.0) ls += w * vad::train_bce(pf, lab);
            s.dz = vad::train_dz(pf, lab, w, denom);
            dzs[n] = s.dz;
        }
        row_loss[b] = ls;
        std::vector<double> dc(H, 0.0), dh(H, 0.0), dg(G, 0.0);
        for (long t = nc - 1; t >= 0; --t) {
            const size_t n = (size_t)b * T + t;
            const Step &s = st[t];
            for (int k = 0; k < H; ++k) {
                double v = 0.0;
                if (t + 1 < nc)
                    for (int j = 0; j < G; ++j) v += p->w_hh[(size_t)j * H + k] * dg[j];
                const double kk = keep ? (keep[n * H + k] ? ks : 0.0) : 1.0;
                dh[k] = (s.h[k] > 0.0 ? kk * p->w_out[k] * s.dz : 0.0) + v;
            }
            for (int k = 0; k < H; ++k) {
                const double i = s.a[k], f = s.a[H + k], gg = s.a[2 * H + k], o = s.a[3 * H + k];
                const double cp = t > 0 ? st[t - 1].c[k] : 0.0;
                const double d_o = dh[k] * s.tc[k];
                const double d_c = dh[k] * o * (1.0 - s.tc[k] * s.tc[k]) + dc[k];
                dg[k] = d_c * gg * i * (1.0 - i);
                dg[H + k] = d_c * cp * f * (1.0 - f);
                dg[2 * H + k] = d_c * i * (1.0 - gg * gg);
                dg[3 * H + k] = d_o * o * (1.0 - o);
                dc[k] = d_c * f;
            }
            std::memcpy(&dG[n * G], dg.data(), G * sizeof(double));
        }
    });

    double total = 0.0;
    for (int b = 0; b < B; ++b) total += row_loss[b];
    *loss = total / denom;

    run_parallel(G, nt, [&](long j) {
        double *wi = g->w_ih + (size_t)j * H, *wh = g->w_hh + (size_t)j * H;
        double sb = 0.0;
        for (int k = 0; k < H; ++k) wi[k] = wh[k] = 0.0;
        for (int b = 0; b < B; ++b)
            for (long t = 0; t < n_chunks[b]; ++t) {
                const size_t n = (size_t)b * T + t;
                const double d = dG[n * G + j];
                const float *x = feat + n * H;
                sb += d;
                for (int k = 0; k < H; ++k) wi[k] += d * (double)x[k];
                if (t > 0)
                    for (int k = 0; k < H; ++k) wh[k] += d * hs[(n - 1) * H + k];
            }
        g->b_ih[j] = g->b_hh[j] = sb;
    });
    double sz = 0.0;
    for (int k = 0; k < H; ++k) g->w_out[k] = 0.0;
    for (int b = 0; b < B; ++b)
        for (long t = 0; t < n_chunks[b]; ++t) {
            const size_t n = (size_t)b * T + t;
            sz += dzs[n];
            for (int k = 0; k < H; ++k) g->w_out[k] += dzs[n] * ys[n * H + k];
        }
    g->b_out[0] = sz;
    return VAD_OK;
}
