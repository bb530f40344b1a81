// The host twin of the augmentations (csrc/augment.cpp, alone) under AddressSanitizer and UBSan, as a stand-alone host program: one row
// of each op, and of a three-op recipe, at len 1, 255, 256 and 257, in buffers that are exactly as long as the call may touch.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/augment_asan.cpp silero_vad_amd/csrc/augment.cpp -pthread -o augment_asan && ./augment_asan
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "silero_vad_hip.h"

static int run(const vad_augment_recipe &r, long len, size_t elem_size) {
    std::vector<int16_t> xi((size_t)len);
    std::vector<float> xf((size_t)len), out((size_t)len, -1.0f);
    for (long i = 0; i < len; ++i) {
        xi[(size_t)i] = (int16_t)(3000.0 * std::sin(0.37 * (double)i));
        xf[(size_t)i] = (float)xi[(size_t)i] / 32768.0f;
    }
    const void *pcm = elem_size == 2 ? (const void *)xi.data() : (const void *)xf.data();
    const int rc = vad_augment_rows_host(pcm, elem_size, len, &len, 1, &r, out.data(), len, 2);
    if (rc) return rc;
    for (long i = 0; i < len; ++i)
        if (!std::isfinite(out[(size_t)i])) return 100;
    return 0;
}

int main() {
    vad_augment_op noise{}, filt{}, clip{};
    noise.kind = VAD_AUGMENT_NOISE;
    noise.a = 0.01;
    noise.seed = 42;
    filt.kind = VAD_AUGMENT_BIQUADS;
    filt.n_sections = VAD_AUGMENT_MAX_SECTIONS;
    for (int s = 0; s < VAD_AUGMENT_MAX_SECTIONS; ++s)
        if (vad_biquad_design(s % 7, 16000.0, 100.0 * (s + 1), 0.7 + 0.1 * s, s % 2 ? 6.0 : -6.0, filt.coef[s])) return 2;
    clip.kind = VAD_AUGMENT_CLIP;
    clip.a = 0.1;
    clip.b = 0.9;
    const vad_augment_op ops[3] = {noise, filt, clip};
    const long lens[4] = {1, 255, 256, 257};
    for (long len : lens)
        for (size_t elem_size : {(size_t)2, (size_t)4}) {
            for (int k = 0; k < 4; ++k) {
                vad_augment_recipe r{};
                r.row_key = 7;
                if (k < 3) {
                    r.n_ops = 1;
                    r.ops[0] = ops[k];
                } else {
                    r.n_ops = 3;
                    std::memcpy(r.ops, ops, sizeof(ops));
                }
                const int rc = run(r, len, elem_size);
                if (rc) {
                    std::fprintf(stderr, "len %ld elem %zu case %d: %d\n", len, elem_size, k, rc);
                    return 1;
                }
            }
        }
    vad_augment_recipe bad{};
    bad.n_ops = 4;
    const char *why = nullptr;
    if (vad_augment_check_recipes(&bad, 1, &why) != VAD_ERR_ARG || !why || !*why) return 3;
    std::puts("augment_asan OK");
    return 0;
}
