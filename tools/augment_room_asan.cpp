// The host twin of the room and aliasing augmentations (csrc/augment.cpp, alone: vad_augment_rows_host_x, vad_rir_shoebox,
// vad_augment_check_recipes_bank) under AddressSanitizer and UBSan, as a stand-alone host program: FIR with 1, 2, 17, 255 and 8192 taps
// out of a bank in which the response is the last thing (so that a read behind it is a read behind the allocation), ALIAS at four
// rates, and both beside a filter, at len 1, 2, 3, 255, 256, 257 and 773, in buffers that are exactly as long as the call may touch;
// the shoebox response at 1, 2, 64 and 8192 taps in a buffer of exactly that many; every refusal.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/augment_room_asan.cpp silero_vad_amd/csrc/augment.cpp -pthread -o augment_room_asan && ./augment_room_asan
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "silero_vad_hip.h"

static int run(const vad_augment_recipe &r, long len, size_t elem_size, const std::vector<float> &bank) {
    std::vector<int16_t> xi((size_t)len);
    std::vector<float> xf((size_t)len), out((size_t)len, -1.0f);
    for (long i = 0; i < len; ++i) {
        xi[(size_t)i] = (int16_t)(3000.0 * std::sin(0.37 * (double)i));
        xf[(size_t)i] = (float)xi[(size_t)i] / 32768.0f;
    }
    const void *pcm = elem_size == 2 ? (const void *)xi.data() : (const void *)xf.data();
    const int rc = vad_augment_rows_host_x(pcm, elem_size, len, &len, 1, &r, out.data(), len, bank.empty() ? nullptr : bank.data(), (long)bank.size(), 2);
    if (rc) return rc;
    for (long i = 0; i < len; ++i)
        if (!std::isfinite(out[(size_t)i])) return 100;
    return 0;
}

int main() {
    const long lens[7] = {1, 2, 3, 255, 256, 257, 773};
    const int taps[5] = {1, 2, 17, 255, VAD_AUGMENT_MAX_TAPS};
    const double rates[4] = {3000.0, 8000.0, 15999.0, 16000.0};
    vad_augment_op filt{};
    filt.kind = VAD_AUGMENT_BIQUADS;
    filt.n_sections = 1;
    if (vad_biquad_design(VAD_BIQUAD_LOWPASS, 16000.0, 2000.0, 0.7, 0.0, filt.coef[0])) return 2;
    for (long len : lens)
        for (size_t elem_size : {(size_t)2, (size_t)4}) {
            for (int K : taps) {
                std::vector<float> bank((size_t)K + 3);                              // the response ends where the bank ends
                for (size_t i = 0; i < bank.size(); ++i) bank[i] = 0.5f * (float)std::cos(0.11 * (double)i) / (float)(1 + i % 7);
                vad_augment_recipe r{};
                r.row_key = 7;
                r.n_ops = 3;
                r.ops[0].kind = VAD_AUGMENT_FIR;
                r.ops[0].n_sections = K;
                r.ops[0].seed = 3;
                r.ops[1] = filt;
                r.ops[2].kind = VAD_AUGMENT_ALIAS;
                r.ops[2].a = rates[K % 4];
                r.ops[2].b = 16000.0;
                int rc = run(r, len, elem_size, bank);
                if (rc) {
                    std::fprintf(stderr, "len %ld elem %zu taps %d: %d\n", len, elem_size, K, rc);
                    return 1;
                }
                r.ops[0].seed = 4;                                                   // one tap behind the bank
                const char *why = nullptr;
                if (vad_augment_check_recipes_bank(&r, 1, (long)bank.size(), &why) != VAD_ERR_ARG || !why || !*why) return 3;
                if (run(r, len, elem_size, bank) != VAD_ERR_ARG) return 4;
            }
            for (double rate : rates) {
                vad_augment_recipe r{};
                r.n_ops = 2;
                r.ops[0].kind = VAD_AUGMENT_ALIAS;
                r.ops[0].a = rate;
                r.ops[0].b = 16000.0;
                r.ops[1] = r.ops[0];
                r.ops[1].a = 0.5 * rate;
                if (run(r, len, elem_size, std::vector<float>())) return 5;
                if (vad_augment_check_recipes(&r, 1, nullptr) != VAD_ERR_ARG) return 6;      // without a bank: an unknown kind
            }
        }
    const double room[3] = {4.7, 3.8, 2.6}, src[3] = {1.1, 2.9, 1.5}, mic[3] = {3.2, 0.9, 1.2}, out_of_room[3] = {4.8, 1.0, 1.0};
    for (long n : {1L, 2L, 64L, (long)VAD_AUGMENT_MAX_TAPS}) {
        std::vector<float> h((size_t)n, -1.0f);
        if (vad_rir_shoebox(16000.0, room, src, mic, 0.2, n == VAD_AUGMENT_MAX_TAPS ? 12 : 4, h.data(), n)) return 7;
        if (!(h[0] >= 1.0f)) return 8;
        for (float v : h)
            if (!std::isfinite(v)) return 9;
    }
    float one = 0.0f;
    if (vad_rir_shoebox(16000.0, room, src, mic, 0.2, 0, &one, 1) || one != 1.0f) return 10;
    if (vad_rir_shoebox(16000.0, room, out_of_room, mic, 0.2, 2, &one, 1) != VAD_ERR_ARG) return 11;
    if (vad_rir_shoebox(16000.0, room, src, src, 0.2, 2, &one, 1) != VAD_ERR_ARG) return 12;
    if (vad_rir_shoebox(16000.0, room, src, mic, 0.0, 2, &one, 1) != VAD_ERR_ARG) return 13;
    if (vad_rir_shoebox(16000.0, room, src, mic, 0.2, 2, &one, 0) != VAD_ERR_ARG) return 14;
    if (vad_rir_shoebox(16000.0, room, src, mic, 0.2, 2, &one, VAD_AUGMENT_MAX_TAPS + 1) != VAD_ERR_ARG) return 15;
    std::puts("augment_room_asan OK");
    return 0;
}
