// WAV sample formats <-> float, one statement of the arithmetic for the host (pcm_host.cpp: vr_pcm_convert_host,
// vr_pcm16_from_float_host) and for the device (stft.hip: the PCM instantiations of stft_tile_kernel / istft_tile_kernel).
//   encode  pcm16_from_float: clip(rint(x * 32767), -32768, 32767), round-half-even -- audio.write, which restates libsndfile's
//           float -> PCM_16 path (f2s_array: scale by 0x7FFF, round to nearest; the clip is a guard).  +-inf clip; NaN gives 0 (numpy's
//           result for NaN is platform-defined, so this is a choice of this library).
//   decode  audio._decode's expressions: PCM16 v / 32768, PCM24 little-endian sign-extended / 2^23, PCM32 (float)((double)v / 2^31),
//           IEEE float32 as stored.  The divisions are by powers of two, so every form of them is exact; only the PCM32 narrowing rounds.
// Samples are interleaved frames of 1 or 2 channels; a mono file is up-mixed by reading the one sample for both network channels
// (inference.py:143-145, np.asarray([X, X])).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vr_mi355.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_PCM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define VR_PCM_HD inline
#endif

namespace vr {

VR_PCM_HD int pcm_sample_bytes(int fmt) { return fmt == VR_PCM_S16 ? 2 : fmt == VR_PCM_S24 ? 3 : 4; }
VR_PCM_HD bool pcm_fmt_ok(int fmt) { return fmt == VR_PCM_S16 || fmt == VR_PCM_S24 || fmt == VR_PCM_S32 || fmt == VR_PCM_F32; }

VR_PCM_HD int16_t pcm16_from_float(float x) {
    const float r = rintf(x * 32767.0f);                // (round-half-even in the default rounding mode, as np.rint)
    if (!(r == r)) return 0;                            // NaN
    return (int16_t)(r < -32768.0f ? -32768.0f : r > 32767.0f ? 32767.0f : r);
}

VR_PCM_HD float pcm_s16_to_float(int16_t v) { return (float)v * (1.0f / 32768.0f); }
// v24: the three bytes little-endian in bits 0..23, anything above
VR_PCM_HD float pcm_s24_to_float(uint32_t v24) { return (float)((int32_t)(v24 << 8) >> 8) * (1.0f / 8388608.0f); }
VR_PCM_HD float pcm_s32_to_float(int32_t v) { return (float)((double)v / 2147483648.0); }

// the aligned 32-bit word at `word`, as little-endian bytes
VR_PCM_HD uint32_t pcm_load_word(const uint8_t* word) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t*>(word);
#else
    uint32_t w;
    memcpy(&w, word, 4);
    return w;
#endif
}

// The three bytes at `p` (any alignment) from whole aligned 32-bit words: the word that holds byte 0, and the next one only when the
// sample straddles it -- so every word read holds at least one byte of the sample, never leaves the 4-byte cell of a valid byte (no
// page is touched that the buffer does not touch) and no byte load is issued.  The device form; the host reads the bytes.
VR_PCM_HD uint32_t pcm_load24(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned sh = (unsigned)(a & 3u) * 8u;
    const uint8_t* w = reinterpret_cast<const uint8_t*>(a & ~uintptr_t(3));
    uint64_t q = pcm_load_word(w);
    if (sh > 8u) q |= (uint64_t)pcm_load_word(w + 4) << 32;
    return (uint32_t)(q >> sh) & 0xffffffu;
#else
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
#endif
}

// sample `i` of channel `ch` (ch < channels) of interleaved frames; PCM16 / PCM32 / F32 need their natural alignment
VR_PCM_HD float pcm_decode(const uint8_t* bytes, int fmt, int channels, long long i, int ch) {
    const long long k = i * channels + ch;
    if (fmt == VR_PCM_S16) {
#if defined(__HIP_DEVICE_COMPILE__)
        return pcm_s16_to_float(reinterpret_cast<const int16_t*>(bytes)[k]);
#else
        int16_t v;
        memcpy(&v, bytes + 2 * k, 2);
        return pcm_s16_to_float(v);
#endif
    }
    if (fmt == VR_PCM_S24) return pcm_s24_to_float(pcm_load24(bytes + 3 * k));
    const uint32_t w = pcm_load_word(bytes + 4 * k);
    if (fmt == VR_PCM_S32) return pcm_s32_to_float((int32_t)w);
    float f;
    memcpy(&f, &w, 4);
    return f;
}

}  // namespace vr
