// Stand-alone walk over the edge values of csrc/pcm.h's host functions, meant for a sanitizer build (not loaded into Python):
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       vocal-remover_amd/csrc/pcm_host.cpp tools/pcm_edge_main.cpp -o tools/_build/pcm_edge && tools/_build/pcm_edge
// Buffers are heap blocks of exactly the bytes a call may touch, at every byte offset, so a read or write past either end is caught.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/vr_mi355.h"

static int fails = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } \
    } while (0)

int main() {
    // ---- encode: ties in both directions, both clip edges, zeros, denormals, infinities, NaN
    std::vector<float> x;
    for (int k = -32769; k <= 32768; ++k)
        for (float d : {-0.5f, 0.f, 0.5f}) x.push_back(((float)k + d) / 32767.0f);
    const float inf = std::numeric_limits<float>::infinity();
    for (float s : {0.f, -0.f, 1e-45f, -1e-45f, 1e-39f, 3.4e38f, -3.4e38f, inf, -inf, std::nanf(""), 1.5f, -1.5f}) x.push_back(s);
    std::vector<int16_t> out(x.size());
    EXPECT(vr_pcm16_from_float_host(x.data(), (int64_t)x.size(), out.data()) == VR_OK);
    for (size_t i = 0; i < x.size(); ++i) {
        const float r = std::nearbyintf(x[i] * 32767.0f);
        const int want = std::isnan(r) ? 0 : r < -32768.f ? -32768 : r > 32767.f ? 32767 : (int)r;
        EXPECT(out[i] == want);
    }
    EXPECT(vr_pcm16_from_float_host(nullptr, 0, nullptr) == VR_OK);
    EXPECT(vr_pcm16_from_float_host(nullptr, 1, out.data()) == VR_ERR_BAD_ARGUMENT);
    // ---- decode: every format, 1 and 2 channels, frame counts around the word sizes, every byte offset of the buffer
    const int fmts[4] = {VR_PCM_S16, VR_PCM_S24, VR_PCM_S32, VR_PCM_F32}, width[4] = {2, 3, 4, 4};
    for (int f = 0; f < 4; ++f)
        for (int ch = 1; ch <= 2; ++ch)
            for (int frames : {0, 1, 2, 3, 5, 1023})
                for (int off = 0; off < 4; ++off) {
                    const size_t nb = (size_t)frames * ch * width[f];
                    unsigned char* block = static_cast<unsigned char*>(std::malloc(nb + off + 1));
                    unsigned char* b = block + off;
                    for (size_t i = 0; i < nb; ++i) b[i] = (unsigned char)(i * 131u + 7u * (unsigned)f + (i >> 3));
                    if (nb >= 12) {               // the extreme codes of the format (float: finite values)
                        const unsigned char lo[4][4] = {{0x00, 0x80}, {0x00, 0x00, 0x80}, {0x00, 0x00, 0x00, 0x80}, {0x00, 0x00, 0x80, 0xbf}};
                        const unsigned char hi[4][4] = {{0xff, 0x7f}, {0xff, 0xff, 0x7f}, {0xff, 0xff, 0xff, 0x7f}, {0x00, 0x00, 0x80, 0x3f}};
                        std::memcpy(b, lo[f], width[f]);
                        std::memcpy(b + width[f], hi[f], width[f]);
                    }
                    float* planar = static_cast<float*>(std::malloc(sizeof(float) * (size_t)frames * ch + 1));
                    // (a shifted copy: the block's last valid byte is the buffer's last byte)
                    unsigned char* tight = static_cast<unsigned char*>(std::malloc(nb ? nb : 1));
                    std::memcpy(tight, b, nb);
                    EXPECT(vr_pcm_convert_host(fmts[f], nb ? tight : nullptr, frames, ch, planar) == VR_OK || frames == 0);
                    float* again = static_cast<float*>(std::malloc(sizeof(float) * (size_t)frames * ch + 1));
                    EXPECT(vr_pcm_convert_host(fmts[f], b, frames, ch, again) == VR_OK);
                    EXPECT(std::memcmp(planar, again, sizeof(float) * (size_t)frames * ch) == 0);
                    if (nb >= 12 && f < 3) { EXPECT(planar[0] == -1.0f); EXPECT(planar[ch == 1 ? 1 : frames] <= 1.0f && planar[ch == 1 ? 1 : frames] > 0.9999f); }
                    std::free(block); std::free(planar); std::free(tight); std::free(again);
                }
    EXPECT(vr_pcm_convert_host(9, nullptr, 0, 2, nullptr) == VR_ERR_BAD_ARGUMENT);
    std::printf(fails ? "pcm_edge: %d FAILED\n" : "pcm_edge: all checks passed\n", fails);
    return fails ? 1 : 0;
}
