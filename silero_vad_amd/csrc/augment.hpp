// augment.hpp -- the audio augmentation rule of decoder fine-tuning (the reference runs audiomentations over every training recording,
// tuning/utils.py:87-143).  Written once for the host twin (augment.cpp, vad_augment_rows_host) and the kernels (kernel_augment.hip).
//
// A row's recipe is an ordered list of 0 .. 3 ops, each applied to the float32 output of the one before; the input is int16
// (x / 32768, the trainer's rule) or float32.  Samples at and behind len are written as zero.
//   NOISE   (a = amplitude, seed)    y[n] = float(double(x[n]) + double(float(a)) * double(g(seed, row_key, n)))
//           g: Philox4x32-10, key = seed (low word, high word), counter = (n / 4 low, n / 4 high, row_key low, row_key high); the four
//           output words give samples 4 k .. 4 k + 3: Box-Muller in double on (w0, w1) -> cos, sin branch, on (w2, w3) -> cos, sin,
//           u = (w + 0.5) 2^-32, g = float(sqrt(-2 log u1) cos / sin (2 pi u2)).  The product of two float32 is exact in double, so
//           the only difference between twin and device is the library's log / cos / sin in double, rounded to float32 once.
//   BIQUADS (n_sections 1 .. 8, coef[s] = b0 b1 b2 a1 a2, a0 = 1)   the cascade in transposed direct form II, in double, zero state:
//           y = b0 x + s0;  s0 = b1 x - a1 y + s1;  s1 = b2 x - a2 y      (scipy.signal.sosfilt's statements), rounded to float32 at
//           the cascade's end.
//   CLIP    (a = q_lo, b = q_hi)     lo, hi = the quantiles of the row's own len samples, numpy's default ("linear") method in double:
//           virtual index v = len q + (1 - q) - 1, neighbours floor(v) and floor(v) + 1, numpy's _lerp, rounded to float32;
//           y = x < lo ? lo : x > hi ? hi : x (a NaN sample stays).  Order is that of the order-preserving uint32 key below, so that
//           NaNs and infinities have a place and twin and device agree on it.
//   ALIAS   (a = new sample rate, b = the row's, 0 < a <= b)   audiomentations' Aliasing as two np.interp calls, n = len:
//           x = linspace(0, n, n), m = rint(n a / b) (half to even), dx = linspace(0, n, m), y = float(interp(x, dx, interp(dx, x, s)));
//           numpy's statements in double without contraction (aug_alias_sample below); n < 2 or m < 2 leaves the row as it is.
//   FIR     (n_sections = K taps, 1 .. 8192, seed = index of tap 0 in the float32 bank beside the recipes)   causal from zero state,
//           y[n] = sum over k = 0 .. min(n, K - 1) of h[k] x[n - k], the output as long as the input.  Twin: exact products summed in
//           double in ascending k, rounded once.  Device: a float32 fmaf chain in ascending k (kernel_augment_x.hip), so that
//           |device - twin| <= (K + 2) 2^-24 sum |h[k]| |x[n - k]|; K = 1 and a single tap of 1.0 are bit-equal.
//   ALIAS and FIR exist for the _x entry points only (vad_augment_rows_device_x / _host_x, vad_augment_check_recipes_bank); the
//   entry points without a bank keep refusing them as unknown kinds.  Neither runs in place: the device call takes a second row
//   buffer (vad_augment_scratch_bytes).
// A row whose final result holds a non-finite value comes back as its input converted to float32 (the reference's add_augs returns
// the original wav on NaN); so does a row whose recipe is empty or invalid.
//
// Device workspace (vad_augment_workspace_bytes(n, width)), nb = ceil(width / kAugBlock):
//   len[n] long | n_ops[n] int | flag[n] int | state[n][nb][16] double, each part rounded up to 256 bytes.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/silero_vad_hip.h"

#if defined(__HIPCC__)
#define VAD_AUG_HD __host__ __device__
#else
#define VAD_AUG_HD
#endif

#ifndef VAD_AUG_BLOCK
#define VAD_AUG_BLOCK 256
#endif

namespace vad {

constexpr int kAugMaxOps = VAD_AUGMENT_MAX_OPS;
constexpr int kAugMaxSections = VAD_AUGMENT_MAX_SECTIONS;
constexpr int kAugStates = 2 * kAugMaxSections;    // doubles of one cascade state
constexpr int kAugMaxTaps = VAD_AUGMENT_MAX_TAPS;
constexpr int kAugBlock = VAD_AUG_BLOCK;           // samples of one block of the three-pass cascade (profiles/augment.md)
static_assert(kAugBlock % 32 == 0 && kAugBlock >= 32, "a block is a whole number of 32-sample tiles");

struct AugLayout {
    size_t len, n_ops, flag, state, total;         // byte offsets
    long nb;                                       // blocks per row
};
VAD_AUG_HD inline size_t aug_up(size_t x) { return (x + 255) / 256 * 256; }
VAD_AUG_HD inline AugLayout aug_layout(long n, long width) {
    AugLayout l{};
    l.nb = (width + kAugBlock - 1) / kAugBlock;
    size_t at = 0;
    l.len = at;    at += aug_up((size_t)n * 8);
    l.n_ops = at;  at += aug_up((size_t)n * 4);
    l.flag = at;   at += aug_up((size_t)n * 4);
    l.state = at;  at += aug_up((size_t)n * (size_t)l.nb * kAugStates * 8);
    l.total = at;
    return l;
}

VAD_AUG_HD inline bool aug_finite(double v) { return v - v == 0.0; }

// 0 = fine, else the index of the sentence in aug_why().  bank_len < 0: the entry points without a bank, to which FIR and ALIAS
// are unknown kinds.
VAD_AUG_HD inline int aug_check(const vad_augment_recipe &r, long bank_len = -1) {
    if (r.n_ops < 0 || r.n_ops > kAugMaxOps) return 1;
    for (int p = 0; p < r.n_ops; ++p) {
        const vad_augment_op &o = r.ops[p];
        if (o.kind == VAD_AUGMENT_NOISE) {
            if (!aug_finite(o.a)) return 5;
        } else if (o.kind == VAD_AUGMENT_BIQUADS) {
            if (o.n_sections < 1 || o.n_sections > kAugMaxSections) return 2;
            for (int s = 0; s < o.n_sections; ++s)
                for (int c = 0; c < 5; ++c)
                    if (!aug_finite(o.coef[s][c])) return 3;
        } else if (o.kind == VAD_AUGMENT_CLIP) {
            if (!(o.a >= 0.0 && o.b <= 1.0 && o.a <= o.b)) return 4;
        } else if (o.kind == VAD_AUGMENT_FIR && bank_len >= 0) {
            if (o.n_sections < 1 || o.n_sections > kAugMaxTaps) return 7;
            if (o.seed > (uint64_t)bank_len || (uint64_t)o.n_sections > (uint64_t)bank_len - o.seed) return 8;
        } else if (o.kind == VAD_AUGMENT_ALIAS && bank_len >= 0) {
            if (!(aug_finite(o.a) && aug_finite(o.b) && o.a > 0.0 && o.a <= o.b)) return 9;
        } else {
            return 6;
        }
    }
    return 0;
}
inline const char *aug_why(int code) {
    static const char *const text[] = {"", "n_ops outside 0 .. 3", "n_sections outside 1 .. 8", "a non-finite filter coefficient",
                                       "quantiles must satisfy 0 <= q_lo <= q_hi <= 1", "a non-finite noise amplitude", "unknown op kind",
                                       "fir taps outside 1 .. 8192", "fir taps outside the bank", "aliasing rates must satisfy 0 < new rate <= rate"};
    return text[code];
}

// ---- NOISE -----------------------------------------------------------------------------------------------------------------------
VAD_AUG_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four standard normals of samples 4 q .. 4 q + 3
VAD_AUG_HD inline void aug_gauss4(uint64_t seed, uint64_t row_key, uint64_t q, float g[4]) {
    uint32_t w[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)row_key, (uint32_t)(row_key >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double k = 1.0 / 4294967296.0, two_pi = 6.283185307179586476925286766559;
    for (int h = 0; h < 2; ++h) {
        const double u1 = ((double)w[2 * h] + 0.5) * k, u2 = ((double)w[2 * h + 1] + 0.5) * k;
        const double r = sqrt(-2.0 * log(u1)), a = two_pi * u2;
        g[2 * h] = (float)(r * cos(a));
        g[2 * h + 1] = (float)(r * sin(a));
    }
}
VAD_AUG_HD inline float aug_add_noise(float x, float amplitude, float g) { return (float)((double)x + (double)amplitude * (double)g); }

// ---- BIQUADS ---------------------------------------------------------------------------------------------------------------------
// one sample through NS sections; c[s] = b0 b1 b2 a1 a2, st[2 s], st[2 s + 1] the section's two states
template <int NS>
VAD_AUG_HD inline double aug_cascade_step(const double (*c)[5], double *st, double x) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double y = c[s][0] * x + st[2 * s];
        st[2 * s] = c[s][1] * x - c[s][3] * y + st[2 * s + 1];
        st[2 * s + 1] = c[s][2] * x - c[s][4] * y;
        x = y;
    }
    return x;
}

// ---- CLIP ------------------------------------------------------------------------------------------------------------------------
// float32 bits -> a uint32 that orders like the value (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN) and back
VAD_AUG_HD inline uint32_t aug_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
VAD_AUG_HD inline uint32_t aug_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// numpy's "linear" quantile of n >= 1 values: the two ranks and the weight of the upper one
VAD_AUG_HD inline void aug_quantile_pos(long n, double q, long *prev, long *next, double *gamma) {
#pragma clang fp contract(off)
    const double v = (double)n * q + (1.0 + q * -1.0) - 1.0;
    if (v >= (double)(n - 1)) {
        *prev = *next = n - 1;
        *gamma = v - floor(v);
    } else if (v < 0.0) {
        *prev = *next = 0;
        *gamma = v - floor(v);
    } else {
        const double f = floor(v);
        *prev = (long)f;
        *next = (long)f + 1;
        *gamma = v - f;
    }
}
// numpy's _lerp(a, b, t), in double, rounded to float32
VAD_AUG_HD inline float aug_lerp(float a, float b, double t) {
#pragma clang fp contract(off)
    const double da = (double)a, db = (double)b, diff = db - da;
    double r = da + diff * t;
    if (t >= 0.5) r = db - diff * (1.0 - t);
    return (float)r;
}
VAD_AUG_HD inline float aug_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- ALIAS -----------------------------------------------------------------------------------------------------------------------
// numpy's linspace(0, n, num)[i] with step = n / (num - 1)
VAD_AUG_HD inline double aug_grid(long i, long num, double step, double n) {
#pragma clang fp contract(off)
    return i == num - 1 ? n : (double)i * step;
}
// the j in [0, num - 2] with grid[j] <= q < grid[j + 1], for 0 <= q < grid[num - 1]: the quotient, corrected by at most one step
VAD_AUG_HD inline long aug_grid_find(double q, long num, double step, double n) {
#pragma clang fp contract(off)
    long j = (long)floor(q / step);
    if (j < 0) j = 0;
    if (j > num - 2) j = num - 2;
    if (j > 0 && aug_grid(j, num, step, n) > q) --j;
    else if (j < num - 2 && aug_grid(j + 1, num, step, n) <= q) ++j;
    return j;
}
// numpy's interp on a grid: the value at q of the line through (grid[j], f0) and (grid[j + 1], f1)
VAD_AUG_HD inline double aug_interp_cell(double q, double x0, double x1, double f0, double f1) {
#pragma clang fp contract(off)
    if (q == x0) return f0;
    return ((f1 - f0) / (x1 - x0)) * (q - x0) + f0;
}
// the new length of an ALIAS op: 0 when the op leaves the row as it is
VAD_AUG_HD inline long aug_alias_m(long n, double a, double b) {
#pragma clang fp contract(off)
    if (n < 2) return 0;
    const double m = rint((double)n * a / b);
    return m < 2.0 ? 0 : (long)m;
}
struct AugAlias {
    long n, m;
    double dn, step_x, step_d;
};
VAD_AUG_HD inline AugAlias aug_alias_plan(long n, long m) {
#pragma clang fp contract(off)
    AugAlias p;
    p.n = n; p.m = m; p.dn = (double)n;
    p.step_x = p.dn / (double)(n - 1);
    p.step_d = p.dn / (double)(m - 1);
    return p;
}
// interp(dx[k], x, s) in double: the inner call, sample k of the row at the new rate
VAD_AUG_HD inline double aug_alias_inner(const AugAlias &p, const float *s, long k) {
#pragma clang fp contract(off)
    const double q = aug_grid(k, p.m, p.step_d, p.dn);
    if (q >= p.dn) return (double)s[p.n - 1];
    const long j = aug_grid_find(q, p.n, p.step_x, p.dn);
    return aug_interp_cell(q, aug_grid(j, p.n, p.step_x, p.dn), aug_grid(j + 1, p.n, p.step_x, p.dn), (double)s[j], (double)s[j + 1]);
}
// output sample i of the ALIAS op over the row s[0 .. n): four input samples, no intermediate array
VAD_AUG_HD inline float aug_alias_sample(const AugAlias &p, const float *s, long i) {
#pragma clang fp contract(off)
    const double q = aug_grid(i, p.n, p.step_x, p.dn);
    if (q >= p.dn) return (float)aug_alias_inner(p, s, p.m - 1);
    const long k = aug_grid_find(q, p.m, p.step_d, p.dn);
    const double x0 = aug_grid(k, p.m, p.step_d, p.dn);
    const double f0 = aug_alias_inner(p, s, k);
    if (q == x0) return (float)f0;
    return (float)aug_interp_cell(q, x0, aug_grid(k + 1, p.m, p.step_d, p.dn), f0, aug_alias_inner(p, s, k + 1));
}

}  // namespace vad
