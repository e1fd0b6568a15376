// vr_pcm_convert_host / vr_pcm16_from_float_host: csrc/pcm.h compiled for the host, so that the arithmetic of the device's sample-format
// kernels can be checked without a GPU (tests/test_cpu_pcm.py, tools/pcm_edge_main.cpp).  No HIP call, no handle.
#include "pcm.h"

extern "C" {

int vr_pcm_convert_host(int fmt, const void* bytes, int64_t frames, int channels, float* planar_out) {
    if (!vr::pcm_fmt_ok(fmt) || channels < 1 || frames < 0 || (frames > 0 && (!bytes || !planar_out))) return VR_ERR_BAD_ARGUMENT;
    const uint8_t* b = static_cast<const uint8_t*>(bytes);
    for (int ch = 0; ch < channels; ++ch)
        for (int64_t i = 0; i < frames; ++i) planar_out[(int64_t)ch * frames + i] = vr::pcm_decode(b, fmt, channels, i, ch);
    return VR_OK;
}

int vr_pcm16_from_float_host(const float* x, int64_t n, int16_t* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return VR_ERR_BAD_ARGUMENT;
    for (int64_t i = 0; i < n; ++i) out[i] = vr::pcm16_from_float(x[i]);
    return VR_OK;
}

}  // extern "C"
