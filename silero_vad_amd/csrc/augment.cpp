// augment.cpp -- vad_augment_rows_host(_x): the rule of augment.hpp on the host, the reference the device call is tested against; the
// recipe check, the filter design and the shoebox room response.  Pure C++.  Rows in parallel, each row by one thread from its first sample to its last (no
// blocks: the same function as the device's three passes, not the same structure), so the result does not depend on `threads`.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/silero_vad_hip.h"
#include "augment.hpp"
#include "host_threads.hpp"

namespace {

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

inline uint32_t bits_of(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}
inline float float_of(uint32_t b) {
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}

// the q-quantile of the keys (which it reorders)
float quantile_of(std::vector<uint32_t> &keys, double q) {
    long prev, next;
    double gamma;
    vad::aug_quantile_pos((long)keys.size(), q, &prev, &next, &gamma);
    std::nth_element(keys.begin(), keys.begin() + prev, keys.end());
    const uint32_t a = keys[(size_t)prev];
    const uint32_t b = next == prev ? a : *std::min_element(keys.begin() + prev + 1, keys.end());
    return vad::aug_lerp(float_of(vad::aug_unkey(a)), float_of(vad::aug_unkey(b)), gamma);
}

template <int NS>
void run_cascade(const vad_augment_op &o, float *y, long len) {
    double c[NS][5], st[2 * NS];
    for (int s = 0; s < NS; ++s)
        for (int k = 0; k < 5; ++k) c[s][k] = o.coef[s][k];
    for (int s = 0; s < 2 * NS; ++s) st[s] = 0.0;
    for (long i = 0; i < len; ++i) y[i] = (float)vad::aug_cascade_step<NS>(c, st, (double)y[i]);
}

// the two ops that cannot run in place: y <- op(y) through a copy of the row
void apply_fir(const vad_augment_op &o, const float *bank, float *y, long len) {
    const long K = o.n_sections;
    const float *h = bank + o.seed;
    const std::vector<float> x(y, y + len);
    for (long n = 0; n < len; ++n) {
        double acc = 0.0;
        const long top = std::min(n, K - 1);
        for (long k = 0; k <= top; ++k) acc += (double)h[k] * (double)x[(size_t)(n - k)];
        y[n] = (float)acc;
    }
}
void apply_alias(const vad_augment_op &o, float *y, long len) {
    const long m = vad::aug_alias_m(len, o.a, o.b);
    if (m == 0) return;
    const std::vector<float> x(y, y + len);
    const vad::AugAlias plan = vad::aug_alias_plan(len, m);
    for (long i = 0; i < len; ++i) y[i] = vad::aug_alias_sample(plan, x.data(), i);
}

void apply_op(const vad_augment_op &o, uint64_t row_key, float *y, long len, const float *bank) {
    if (o.kind == VAD_AUGMENT_FIR) {
        apply_fir(o, bank, y, len);
    } else if (o.kind == VAD_AUGMENT_ALIAS) {
        apply_alias(o, y, len);
    } else if (o.kind == VAD_AUGMENT_NOISE) {
        const float amp = (float)o.a;
        for (long q = 0; 4 * q < len; ++q) {
            float g[4];
            vad::aug_gauss4(o.seed, row_key, (uint64_t)q, g);
            for (int k = 0; k < 4 && 4 * q + k < len; ++k) y[4 * q + k] = vad::aug_add_noise(y[4 * q + k], amp, g[k]);
        }
    } else if (o.kind == VAD_AUGMENT_BIQUADS) {
        switch (o.n_sections) {
            case 1: run_cascade<1>(o, y, len); break;
            case 2: run_cascade<2>(o, y, len); break;
            case 3: run_cascade<3>(o, y, len); break;
            case 4: run_cascade<4>(o, y, len); break;
            case 5: run_cascade<5>(o, y, len); break;
            case 6: run_cascade<6>(o, y, len); break;
            case 7: run_cascade<7>(o, y, len); break;
            default: run_cascade<8>(o, y, len); break;
        }
    } else if (o.kind == VAD_AUGMENT_CLIP && len > 0) {
        std::vector<uint32_t> keys((size_t)len);
        for (long i = 0; i < len; ++i) keys[(size_t)i] = vad::aug_key(bits_of(y[i]));
        const float lo = quantile_of(keys, o.a), hi = quantile_of(keys, o.b);
        for (long i = 0; i < len; ++i) y[i] = vad::aug_clip(y[i], lo, hi);
    }
}

void load_row(const void *pcm, size_t elem_size, long ld, long row, float *y, long len, long width) {
    if (elem_size == 2) {
        const int16_t *x = static_cast<const int16_t *>(pcm) + (size_t)row * ld;
        for (long i = 0; i < len; ++i) y[i] = (float)x[i] / 32768.0f;
    } else {
        const float *x = static_cast<const float *>(pcm) + (size_t)row * ld;
        for (long i = 0; i < len; ++i) y[i] = x[i];
    }
    for (long i = len; i < width; ++i) y[i] = 0.0f;
}

// the distance from the microphone to the image of the source with reflection counts n and parities p (Allen and Berkley)
double image_distance(const int n[3], const int p[3], const double room[3], const double src[3], const double mic[3]) {
#pragma clang fp contract(off)
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double im = (2.0 * (double)n[a]) * room[a] + (double)(1 - 2 * p[a]) * src[a];
        const double e = im - mic[a];
        d2 = d2 + e * e;
    }
    return std::sqrt(d2);
}
// one image into the response: amplitude gain d0 / d at the fractional delay (d - d0) sr / c, split over two taps
void shoebox_add(std::vector<double> &acc, long n_taps, double gain, double d, double d0, double sr, double c) {
#pragma clang fp contract(off)
    const double A = gain * d0 / d, t = (d - d0) * sr / c;
    const double fl = std::floor(t), f = t - fl;
    if (!(fl >= 0.0) || fl >= (double)n_taps) return;                        // (the direct path is the shortest: t >= 0)
    const long j = (long)fl;
    acc[(size_t)j] += A * (1.0 - f);
    if (j + 1 < n_taps) acc[(size_t)j + 1] += A * f;
}

}  // namespace

extern "C" long vad_augment_block(void) { return vad::kAugBlock; }

extern "C" size_t vad_augment_workspace_bytes(long n_rows, long width) {
    if (n_rows <= 0 || width <= 0 || (double)n_rows * (double)width > 4e10) return 0;
    return vad::aug_layout(n_rows, width).total;
}

extern "C" size_t vad_augment_scratch_bytes(long n_rows, long width) {
    if (n_rows <= 0 || width <= 0 || (double)n_rows * (double)width > 4e10) return 0;
    return vad::aug_up((size_t)n_rows * (size_t)width * 4);
}

// bank_len < 0: the check without a bank
static int check_recipes(const vad_augment_recipe *recipes, long n, long bank_len, const char **why) {
    if (why) *why = "";
    if (!recipes || n < 0) {
        if (why) *why = "null recipes";
        return VAD_ERR_ARG;
    }
    for (long i = 0; i < n; ++i) {
        const int code = vad::aug_check(recipes[i], bank_len);
        if (code) {
            if (why) *why = vad::aug_why(code);
            return VAD_ERR_ARG;
        }
    }
    return VAD_OK;
}

extern "C" int vad_augment_check_recipes(const vad_augment_recipe *recipes, long n, const char **why) {
    return check_recipes(recipes, n, -1, why);
}

extern "C" int vad_augment_check_recipes_bank(const vad_augment_recipe *recipes, long n, long bank_len, const char **why) {
    if (bank_len < 0) {
        if (why) *why = "a negative bank length";
        return VAD_ERR_ARG;
    }
    return check_recipes(recipes, n, bank_len, why);
}

// bank_len < 0: no bank, FIR and ALIAS are unknown kinds
static int rows_host(const void *pcm, size_t elem_size, long ld, const long *lens, long n, const vad_augment_recipe *recipes, float *out,
                     long ld_out, const float *bank, long bank_len, int threads) {
    if (!pcm || !lens || !recipes || !out || n <= 0 || ld <= 0 || ld_out <= 0 || (elem_size != 2 && elem_size != 4)) return VAD_ERR_ARG;
    for (long i = 0; i < n; ++i)
        if (lens[i] < 0 || lens[i] > ld || lens[i] > ld_out) return VAD_ERR_ARG;
    const int rc = check_recipes(recipes, n, bank_len, nullptr);
    if (rc) return rc;
    const int nt = threads > 0 ? threads : vad::default_host_threads(64);
    run_parallel(n, nt, [&](long row) {
        const vad_augment_recipe &r = recipes[row];
        float *y = out + (size_t)row * ld_out;
        const long len = lens[row];
        load_row(pcm, elem_size, ld, row, y, len, ld_out);
        if (r.n_ops == 0) return;
        for (int p = 0; p < r.n_ops; ++p) apply_op(r.ops[p], r.row_key, y, len, bank);
        bool finite = true;
        for (long i = 0; i < len && finite; ++i) finite = std::isfinite(y[i]);
        if (!finite) load_row(pcm, elem_size, ld, row, y, len, ld_out);
    });
    return VAD_OK;
}

extern "C" int vad_augment_rows_host(const void *pcm, size_t elem_size, long ld, const long *lens, long n, const vad_augment_recipe *recipes,
                                     float *out, long ld_out, int threads) {
    return rows_host(pcm, elem_size, ld, lens, n, recipes, out, ld_out, nullptr, -1, threads);
}

extern "C" int vad_augment_rows_host_x(const void *pcm, size_t elem_size, long ld, const long *lens, long n, const vad_augment_recipe *recipes,
                                       float *out, long ld_out, const float *fir_bank, long fir_bank_len, int threads) {
    if (fir_bank_len < 0 || (!fir_bank && fir_bank_len > 0)) return VAD_ERR_ARG;
    return rows_host(pcm, elem_size, ld, lens, n, recipes, out, ld_out, fir_bank, fir_bank_len, threads);
}

extern "C" int vad_rir_shoebox(double sr, const double room[3], const double src[3], const double mic[3], double absorption, int max_order,
                               float *h, long n_taps) {
    if (!room || !src || !mic || !h || n_taps < 1 || n_taps > vad::kAugMaxTaps || max_order < 0) return VAD_ERR_ARG;
    if (!std::isfinite(sr) || !(sr > 0.0) || !std::isfinite(absorption) || !(absorption > 0.0) || !(absorption <= 1.0)) return VAD_ERR_ARG;
    bool same = true;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(room[a]) || !(room[a] > 0.0)) return VAD_ERR_ARG;
        if (!(src[a] > 0.0 && src[a] < room[a] && mic[a] > 0.0 && mic[a] < room[a])) return VAD_ERR_ARG;
        same = same && src[a] == mic[a];
    }
    if (same) return VAD_ERR_ARG;
    const double beta = std::sqrt(1.0 - absorption), c = 343.0;
    const int zero[3] = {0, 0, 0};
    const double d0 = image_distance(zero, zero, room, src, mic);
    std::vector<double> acc((size_t)n_taps, 0.0);
    std::vector<double> power((size_t)max_order + 1, 1.0);                   // beta^R, 0^0 = 1
    for (int r = 1; r <= max_order; ++r) power[(size_t)r] = power[(size_t)r - 1] * beta;
    const int N = max_order;
    for (int nx = -N; nx <= N; ++nx)
        for (int ny = -N; ny <= N; ++ny)
            for (int nz = -N; nz <= N; ++nz)
                for (int px = 0; px < 2; ++px)
                    for (int py = 0; py < 2; ++py)
                        for (int pz = 0; pz < 2; ++pz) {
                            const int nn[3] = {nx, ny, nz}, pp[3] = {px, py, pz};
                            int R = 0;
                            for (int a = 0; a < 3; ++a) R += std::abs(nn[a] - pp[a]) + std::abs(nn[a]);
                            if (R > max_order) continue;
                            shoebox_add(acc, n_taps, power[(size_t)R], image_distance(nn, pp, room, src, mic), d0, sr, c);
                        }
    for (long i = 0; i < n_taps; ++i) h[i] = (float)acc[(size_t)i];
    return VAD_OK;
}

extern "C" int vad_biquad_design(int kind, double sr, double f0, double q, double gain_db, double coef[5]) {
    if (!coef || kind < VAD_BIQUAD_LOWPASS || kind > VAD_BIQUAD_HIGHSHELF) return VAD_ERR_ARG;
    if (!std::isfinite(sr) || !std::isfinite(f0) || !std::isfinite(q) || !std::isfinite(gain_db)) return VAD_ERR_ARG;
    if (!(sr > 0.0) || !(f0 > 0.0) || !(f0 < 0.5 * sr) || !(q > 0.0)) return VAD_ERR_ARG;
    const double w0 = 2.0 * M_PI * f0 / sr, cs = std::cos(w0), sn = std::sin(w0), alpha = sn / (2.0 * q);
    const double hs = std::sin(0.5 * w0), hc = std::cos(0.5 * w0);        // 1 - cos w0 = 2 hs^2, 1 + cos w0 = 2 hc^2, without cancellation
    const double A = std::pow(10.0, gain_db / 40.0), rA = 2.0 * std::sqrt(A) * alpha;
    double b0, b1, b2, a0, a1, a2;
    switch (kind) {
        case VAD_BIQUAD_LOWPASS:
            b0 = hs * hs; b1 = 2.0 * hs * hs; b2 = hs * hs; a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case VAD_BIQUAD_HIGHPASS:
            b0 = hc * hc; b1 = -2.0 * hc * hc; b2 = hc * hc; a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case VAD_BIQUAD_BANDPASS:
            b0 = alpha; b1 = 0.0; b2 = -alpha; a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case VAD_BIQUAD_NOTCH:
            b0 = 1.0; b1 = -2.0 * cs; b2 = 1.0; a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
            break;
        case VAD_BIQUAD_PEAKING:
            b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A; a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
            break;
        case VAD_BIQUAD_LOWSHELF:
            b0 = A * ((A + 1.0) - (A - 1.0) * cs + rA); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs); b2 = A * ((A + 1.0) - (A - 1.0) * cs - rA);
            a0 = (A + 1.0) + (A - 1.0) * cs + rA; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs); a2 = (A + 1.0) + (A - 1.0) * cs - rA;
            break;
        default:
            b0 = A * ((A + 1.0) + (A - 1.0) * cs + rA); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs); b2 = A * ((A + 1.0) + (A - 1.0) * cs - rA);
            a0 = (A + 1.0) - (A - 1.0) * cs + rA; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs); a2 = (A + 1.0) - (A - 1.0) * cs - rA;
            break;
    }
    coef[0] = b0 / a0; coef[1] = b1 / a0; coef[2] = b2 / a0; coef[3] = a1 / a0; coef[4] = a2 / a0;
    return VAD_OK;
}
