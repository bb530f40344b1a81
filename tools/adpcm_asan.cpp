// The host twin of the DVI4 decode (csrc/adpcm.hpp adpcm_expand_serial, the body of vad_adpcm_expand) under AddressSanitizer and UBSan,
// as a stand-alone host program: payloads of 4, 5, 84 and 260 bytes -- random codes, and the saturating and index-floor runs -- in
// buffers that are exactly as long as the call may touch, each result compared with the recurrence written out below; then the
// refusals.  Run on the host; it never goes through pytest or onto a GPU machine.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/adpcm_asan.cpp -o adpcm_asan && ./adpcm_asan
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../silero_vad_amd/csrc/adpcm.hpp"

static const int kStep[89] = {7,     8,     9,     10,    11,    12,    13,    14,    16,    17,    19,    21,    23,    25,    28,
                              31,    34,    37,    41,    45,    50,    55,    60,    66,    73,    80,    88,    97,    107,   118,
                              130,   143,   157,   173,   190,   209,   230,   253,   279,   307,   337,   371,   408,   449,   494,
                              544,   598,   658,   724,   796,   876,   963,   1060,  1166,  1282,  1411,  1552,  1707,  1878,  2066,
                              2272,  2499,  2749,  3024,  3327,  3660,  4026,  4428,  4871,  5358,  5894,  6484,  7132,  7845,  8630,
                              9493,  10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
static const int kIdx[8] = {-1, -1, -1, -1, 2, 4, 6, 8};

// one payload of nbytes bytes: header (predict, index, reserved), every code byte from `fill` (0 ... 255) or, with fill < 0, from an LCG
static int run(long nbytes, int predict, int index, int fill, unsigned seed) {
    std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)nbytes]);
    const long n = 2 * (nbytes - 4);
    std::unique_ptr<int16_t[]> out(n ? new int16_t[(size_t)n] : nullptr);
    in[0] = (uint8_t)((unsigned)predict >> 8), in[1] = (uint8_t)predict, in[2] = (uint8_t)index, in[3] = 0xa5;
    for (long i = 4; i < nbytes; ++i) in[i] = fill >= 0 ? (uint8_t)fill : (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    if (vad::adpcm_expand_serial(in.get(), nbytes, out.get()) != n) return 1;
    int pred = predict, idx = index > 88 ? 88 : index;
    for (long j = 0; j < n; ++j) {
        const int d = j & 1 ? in[4 + j / 2] & 15 : in[4 + j / 2] >> 4, step = kStep[idx];
        int v = step >> 3;
        if (d & 4) v += step;
        if (d & 2) v += step >> 1;
        if (d & 1) v += step >> 2;
        pred = d & 8 ? pred - v : pred + v;
        pred = pred < -32768 ? -32768 : pred > 32767 ? 32767 : pred;
        idx += kIdx[d & 7];
        idx = idx < 0 ? 0 : idx > 88 ? 88 : idx;
        if (out[(size_t)j] != pred) return 2;
    }
    return 0;
}

int main() {
    const long sizes[4] = {4, 5, 84, 260};
    for (long nbytes : sizes) {
        const int cases[8][3] = {{0, 0, -1},        {-12345, 40, -1},   {32767, 88, 0x77}, {-32767, 88, 0xff},
                                 {1000, 3, 0x00}, {-1000, 3, 0x88}, {5, 89, -1},       {-5, 255, -1}};
        for (int k = 0; k < 8; ++k) {
            const int rc = run(nbytes, cases[k][0], cases[k][1], cases[k][2], 17u * (unsigned)nbytes + (unsigned)k);
            if (rc) {
                std::fprintf(stderr, "nbytes %ld case %d: %d\n", nbytes, k, rc);
                return 1;
            }
        }
    }
    uint8_t three[3] = {0, 0, 0}, five[5] = {0, 0, 0, 0, 0x17};
    int16_t two[2] = {77, 77};
    if (vad::adpcm_expand_serial(three, 3, two) >= 0 || vad::adpcm_expand_serial(nullptr, 0, nullptr) >= 0 ||
        vad::adpcm_expand_serial(five, -1, two) >= 0)
        return 3;
    if (vad::adpcm_expand_serial(nullptr, 5, two) >= 0 || vad::adpcm_expand_serial(five, 5, nullptr) >= 0 || two[0] != 77 || two[1] != 77) return 4;
    if (vad::adpcm_expand_serial(nullptr, 4, nullptr) != 0 || vad::adpcm_expand_serial(five, 4, nullptr) != 0) return 5;
    if (vad::adpcm_expand_serial(five, 5, two) != 2 || two[0] != 1 || two[1] != 12) return 6;     // step 7: code 1 adds 0 + 1, code 7 adds 0 + 7 + 3 + 1
    std::puts("adpcm_asan OK");
    return 0;
}
