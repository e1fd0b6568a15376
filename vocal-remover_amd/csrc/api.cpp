// extern "C" surface of libvr_mi355.so (include/vr_mi355.h).  Exceptions stop here.
#include "../../include/vr_mi355.h"

#include <cstddef>
#include <cstring>
#include <new>

#include "model.h"

namespace vr {
void resample_api(int device, const float* x, int channels, long long n_in, int sr_in, int sr_out, float* y, long long n_out);
void resample_ratio_api(int device, const float* x, int channels, long long n_in, double ratio, float* y, long long n_out);
void xcorr_argmax_api(int device, const float* a, long long na, const float* b, long long nb, long long* argmax_out);
void align_pair_check(int n, const float* const* mix, const float* const* inst, const long long* L_mix, const long long* L_inst, int sr,
                      const void* out);
void align_pair_many_api(int device, int n, const float* const* mix, const float* const* inst, bool on_dev, const long long* L_mix,
                         const long long* L_inst, int sr, PairWindow* out);
struct Resampler;
long long resampler_plan(int sr_in, int sr_out, long long samples_in, bool flushed);
Resampler* resampler_open(int device, int channels, int sr_in, int sr_out);
void resampler_close(Resampler* r);
void resampler_info(const Resampler* r, long long* lookahead, long long* state_bytes);
void resampler_push_many(int N, Resampler* const* r, const float* const* x, bool x_on_dev, const long long* n, const int* flush,
                         float* const* y, bool y_on_dev, const long long* capacity, long long* n_out, bool many,
                         const void* const* bytes = nullptr, const int* pcm_channels = nullptr, const int* pcm_fmt = nullptr);
}  // namespace vr

struct vr_model {
    vr::Model m;
    vr_model(int d, int n, int h, int o, int l, bool cplx) : m(d, n, h, o, l, cplx) {}
};

static thread_local std::string g_err;

template <class F>
static int guard(F&& f) {
    try {
        f();
        return VR_OK;
    } catch (const vr::Error& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "host allocation failed";
        return VR_ERR_OOM;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VR_ERR_UNKNOWN;
    } catch (...) {
        g_err = "unknown error";
        return VR_ERR_UNKNOWN;
    }
}

#define NEED(h)                                                  \
    if (!(h)) {                                                  \
        g_err = "null handle";                                   \
        return VR_ERR_BAD_ARGUMENT;                              \
    }

extern "C" {

const char* vr_last_error(void) { return g_err.c_str(); }

int vr_create(int device, int n_fft, int hop_length, int nout, int nout_lstm, vr_handle* out) {
    return vr_create_ex(device, n_fft, hop_length, nout, nout_lstm, 0, out);
}

int vr_create_ex(int device, int n_fft, int hop_length, int nout, int nout_lstm, int flags, vr_handle* out) {
    if (!out) { g_err = "null out pointer"; return VR_ERR_BAD_ARGUMENT; }
    *out = nullptr;
    return guard([&] {
        if (flags & ~VR_CREATE_COMPLEX) throw vr::Error(VR_ERR_BAD_ARGUMENT, "unknown vr_create_ex flag");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            throw vr::Error(VR_ERR_HIP, "no HIP device visible: libvr_mi355 has no CPU fallback");
        if (device < 0 || device >= count) throw vr::Error(VR_ERR_BAD_ARGUMENT, "device index out of range");
        *out = new vr_model(device, n_fft, hop_length, nout, nout_lstm, (flags & VR_CREATE_COMPLEX) != 0);
    });
}

int vr_destroy(vr_handle h) {
    NEED(h);
    return guard([&] { delete h; });
}

int vr_num_params(vr_handle h) {
    if (!h) return VR_ERR_BAD_ARGUMENT;
    return (int)h->m.params.size();
}

int vr_param_info(vr_handle h, int index, char* key_buf, int key_cap, int64_t* shape4, int* ndim, int* is_int64,
                  int* trainable) {
    NEED(h);
    return guard([&] {
        VR_CHECK(index >= 0 && index < (int)h->m.params.size(), VR_ERR_BAD_ARGUMENT, "param index out of range");
        const vr::Param& p = h->m.params[index];
        if (key_buf) {
            VR_CHECK((int)p.key.size() + 1 <= key_cap, VR_ERR_BAD_ARGUMENT, "key buffer too small");
            std::memcpy(key_buf, p.key.c_str(), p.key.size() + 1);
        }
        if (ndim) *ndim = (int)p.shape.size();
        if (shape4)
            for (size_t i = 0; i < p.shape.size() && i < 4; ++i) shape4[i] = p.shape[i];
        if (is_int64) *is_int64 = p.kind == vr::PK_NBT;
        if (trainable) *trainable = p.trainable;
    });
}

int vr_set_param(vr_handle h, const char* key, const void* host, const int64_t* shape, int ndim) {
    NEED(h);
    return guard([&] {
        VR_CHECK(key && host && (shape || ndim == 0), VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.set_param(key, host, shape, ndim);
    });
}

int vr_get_param(vr_handle h, const char* key, void* host, int64_t capacity_bytes) {
    NEED(h);
    return guard([&] {
        VR_CHECK(key && host, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.get_param(key, host, capacity_bytes);
    });
}

int vr_set_mode(vr_handle h, int training) {
    NEED(h);
    return guard([&] { h->m.set_training(training != 0); });
}

int vr_set_option(vr_handle h, const char* name, int value) {
    NEED(h);
    return guard([&] {
        VR_CHECK(name, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.set_option(name, value);
    });
}

int vr_set_loss(vr_handle h, int kind, double sdr_weight) {
    NEED(h);
    return guard([&] { h->m.set_loss(kind, sdr_weight); });
}

int vr_get_loss(vr_handle h, int* kind, double* sdr_weight) {
    NEED(h);
    return guard([&] {
        if (kind) *kind = h->m.loss_kind;
        if (sdr_weight) *sdr_weight = h->m.sdr_weight;
    });
}

int vr_loss_terms(vr_handle h, double* mag_l1, double* sdr) {
    NEED(h);
    return guard([&] {
        VR_CHECK(h->m.loss_terms_valid, VR_ERR_BAD_ARGUMENT, "vr_loss_terms: no vr_train_step / vr_validate_step under VR_LOSS_MAG_L1_WAVE_SDR "
                                                             "or VR_LOSS_MAG_L1_WAVE_WSDR on this handle since its loss was set");
        if (mag_l1) *mag_l1 = h->m.last_mag_l1;
        if (sdr) *sdr = h->m.last_sdr;
    });
}

int vr_loss_terms_wsdr(vr_handle h, double* y_sdr, double* noise_sdr, double* alpha) {
    NEED(h);
    return guard([&] {
        VR_CHECK(h->m.loss_terms_valid && h->m.loss_kind == VR_LOSS_MAG_L1_WAVE_WSDR, VR_ERR_BAD_ARGUMENT,
                 "vr_loss_terms_wsdr: no vr_train_step / vr_validate_step under VR_LOSS_MAG_L1_WAVE_WSDR on this handle since its loss was set");
        if (y_sdr) *y_sdr = h->m.last_y_sdr;
        if (noise_sdr) *noise_sdr = h->m.last_noise_sdr;
        if (alpha) *alpha = h->m.last_alpha;
    });
}

int vr_forward(vr_handle h, const float* x, int x_on_device, int B, int T, int mode, float* out, int out_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(x && out, VR_ERR_BAD_ARGUMENT, "null argument");
        VR_CHECK(mode >= 0 && mode <= 2, VR_ERR_BAD_ARGUMENT, "mode must be 0 (forward), 1 (predict_mask) or 2 (predict)");
        h->m.forward_api(x, x_on_device != 0, B, T, mode, out, out_on_device != 0);
    });
}

int vr_stft(vr_handle h, const float* wave, int wave_on_device, int64_t L, float* spec, int spec_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(wave && spec, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.stft_api(wave, wave_on_device != 0, L, spec, spec_on_device != 0);
    });
}

int vr_istft(vr_handle h, const float* spec, int spec_on_device, int T, float* wave, int wave_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(spec && wave, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.istft_api(spec, spec_on_device != 0, T, wave, wave_on_device != 0);
    });
}

int vr_separate(vr_handle h, const float* spec, int spec_on_device, int T, int tta, int batchsize, int cropsize,
                float* y_spec, float* v_spec, int out_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(spec && y_spec && v_spec, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.separate_run(1, &spec, spec_on_device != 0, &T, nullptr, tta, batchsize, cropsize, &y_spec, &v_spec, out_on_device != 0, nullptr,
                          nullptr, /*solo=*/true);
    });
}

int vr_separate_wave(vr_handle h, const float* wave, int wave_on_device, int64_t L, int tta, int batchsize,
                     int cropsize, float* y_wave, float* v_wave, int out_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(wave && y_wave && v_wave, VR_ERR_BAD_ARGUMENT, "null argument");
        const long long len = L;
        h->m.separate_run(1, &wave, wave_on_device != 0, nullptr, &len, tta, batchsize, cropsize, &y_wave, &v_wave, out_on_device != 0, nullptr,
                          nullptr, /*solo=*/true);
    });
}

// The many-song forms check their tables before the handle, so that a caller's argument error is reported without a device.
static bool many_args_ok(int n_songs, const void* in, const void* len, const void* y, const void* v) {
    if (n_songs <= 0) { g_err = "n_songs must be positive"; return false; }
    if (!in || !len || !y || !v) { g_err = "null table"; return false; }
    return true;
}

int vr_separate_many(vr_handle h, int n_songs, const float* const* specs, int specs_on_device, const int* T, int tta, int batchsize,
                     int cropsize, float* const* y_specs, float* const* v_specs, int out_on_device) {
    if (!many_args_ok(n_songs, specs, T, y_specs, v_specs)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        h->m.separate_run(n_songs, specs, specs_on_device != 0, T, nullptr, tta, batchsize, cropsize, y_specs, v_specs,
                          out_on_device != 0);
    });
}

int vr_separate_wave_many(vr_handle h, int n_songs, const float* const* waves, int waves_on_device, const int64_t* L, int tta,
                          int batchsize, int cropsize, float* const* y_waves, float* const* v_waves, int out_on_device) {
    if (!many_args_ok(n_songs, waves, L, y_waves, v_waves)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        std::vector<long long> len(L, L + n_songs);
        h->m.separate_run(n_songs, waves, waves_on_device != 0, nullptr, len.data(), tta, batchsize, cropsize, y_waves, v_waves,
                          out_on_device != 0);
    });
}

// ---- spectrogram images ---------------------------------------------------------------------------------------
// What can be judged without the handle: the count, the tables, a stem table or a picture table without its partner.
static bool image_args_ok(int n_songs, const void* in, const void* len, const void* y, const void* v, const void* y_img, const void* v_img) {
    if (n_songs <= 0) { g_err = "n_songs must be positive"; return false; }
    if (!in || !len) { g_err = "null table"; return false; }
    if ((y == nullptr) != (v == nullptr)) { g_err = "one stem table is null and the other is not: give both, or neither for pictures only"; return false; }
    if ((y_img == nullptr) != (v_img == nullptr)) { g_err = "one picture table is null and the other is not"; return false; }
    if (!y_img) { g_err = "null table"; return false; }
    return true;
}

int vr_separate_wave_many_img(vr_handle h, int n_songs, const float* const* waves, int waves_on_device, const int64_t* L, int tta,
                              int batchsize, int cropsize, float* const* y_waves, float* const* v_waves, int out_on_device,
                              uint8_t* const* y_img, uint8_t* const* v_img, float* ranges) {
    if (!image_args_ok(n_songs, waves, L, y_waves, v_waves, y_img, v_img)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        std::vector<long long> len(L, L + n_songs);
        const vr::ImageArgs im{y_img, v_img, ranges, y_waves != nullptr};
        h->m.separate_run(n_songs, waves, waves_on_device != 0, nullptr, len.data(), tta, batchsize, cropsize, y_waves, v_waves,
                          out_on_device != 0, nullptr, nullptr, /*solo=*/false, nullptr, nullptr, &im);
    });
}

int vr_separate_pcm_many_img(vr_handle h, int n_songs, const void* const* bytes, int on_device, const int64_t* frames, const int* channels,
                             const int* fmt, int tta, int batchsize, int cropsize, int16_t* const* y, int16_t* const* v, int out_on_device,
                             uint8_t* const* y_img, uint8_t* const* v_img, float* ranges) {
    if (!image_args_ok(n_songs, bytes, frames, y, v, y_img, v_img)) return VR_ERR_BAD_ARGUMENT;
    if (!channels || !fmt) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    return guard([&] {
        std::vector<long long> len(frames, frames + n_songs);
        const vr::ImageArgs im{y_img, v_img, ranges, y != nullptr};
        h->m.separate_run(n_songs, reinterpret_cast<const float* const*>(bytes), on_device != 0, nullptr, len.data(), tta, batchsize,
                          cropsize, reinterpret_cast<float* const*>(y), reinterpret_cast<float* const*>(v), out_on_device != 0, channels, fmt,
                          /*solo=*/false, nullptr, nullptr, &im);
    });
}

static void need_device(int device);

int vr_spec_image_many(int device, int n, const void* const* specs, int on_device, int channels, int bins, const int* T, int is_complex,
                       int mode, uint8_t* const* imgs, int out_on_device, float* ranges) {
    if (n <= 0 || !specs || !T || !imgs) { g_err = "spec image: no picture or a null table"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        VR_CHECK(channels == 1 || channels == 2, VR_ERR_BAD_ARGUMENT, "spec image: channels must be 1 or 2");
        VR_CHECK(bins > 0, VR_ERR_BAD_ARGUMENT, "spec image: bins must be positive");
        VR_CHECK(mode == VR_IMAGE_MAGNITUDE || mode == VR_IMAGE_PHASE, VR_ERR_BAD_ARGUMENT, "spec image: unknown mode (VR_IMAGE_MAGNITUDE or VR_IMAGE_PHASE)");
        for (int i = 0; i < n; ++i) {
            const std::string who = "spec image: picture " + std::to_string(i) + ": ";
            VR_CHECK(specs[i] && imgs[i], VR_ERR_BAD_ARGUMENT, who + "null pointer");
            VR_CHECK(T[i] > 0, VR_ERR_BAD_ARGUMENT, who + "T must be positive");
            VR_CHECK((long long)bins * T[i] < (1LL << 31), VR_ERR_BAD_ARGUMENT, who + "more than 2^31 - 1 pixels");
            if (on_device)
                VR_CHECK((reinterpret_cast<uintptr_t>(specs[i]) & (is_complex ? 7 : 3)) == 0, VR_ERR_BAD_ARGUMENT,
                         who + "a device spectrogram needs its natural alignment");
        }
        need_device(device);
        vr::spec_image_many_api(device, n, specs, on_device != 0, channels, bins, T, is_complex != 0, mode, imgs, out_on_device != 0, ranges);
    });
}

int vr_spec_image(int device, const void* spec, int on_device, int channels, int bins, int T, int is_complex, int mode, uint8_t* img,
                  int out_on_device, float* range) {
    if (!spec || !img) { g_err = "spec image: null argument"; return VR_ERR_BAD_ARGUMENT; }
    return vr_spec_image_many(device, 1, &spec, on_device, channels, bins, &T, is_complex, mode, &img, out_on_device, range);
}

// ---- evaluation against the true stems -------------------------------------------------------------------
// What can be judged without the handle is: the tables, the counts, a stem table without its partner, a window or a length below one
// sample.  window < hop and L < hop need the handle's hop: Model::separate_run refuses them before it touches the device.
static bool evaluate_args_ok(int n_songs, const void* mix, const void* inst, const int64_t* L, int64_t window, const void* sums, const void* y,
                             const void* v) {
    if (n_songs <= 0) { g_err = "n_songs must be positive"; return false; }
    if (!mix || !inst || !L || !sums) { g_err = "null table"; return false; }
    if ((y == nullptr) != (v == nullptr)) { g_err = "one stem table is null and the other is not: give both, or neither for sums only"; return false; }
    if (window < 1) { g_err = "window shorter than one hop"; return false; }
    return true;
}

int vr_evaluate_wave_many(vr_handle h, int n_songs, const float* const* mix, const float* const* inst, int on_device, const int64_t* L, int tta,
                          int batchsize, int cropsize, int64_t window, double* const* sums, float* const* y_waves, float* const* v_waves,
                          int out_on_device) {
    if (!evaluate_args_ok(n_songs, mix, inst, L, window, sums, y_waves, v_waves)) return VR_ERR_BAD_ARGUMENT;
    for (int s = 0; s < n_songs; ++s)
        if (L[s] < 1) { g_err = "song " + std::to_string(s) + ": wave shorter than one hop"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    return guard([&] {
        std::vector<long long> len(L, L + n_songs);
        const vr::EvalArgs ev{inst, (long long)window, sums, y_waves != nullptr};
        h->m.separate_run(n_songs, mix, on_device != 0, nullptr, len.data(), tta, batchsize, cropsize, y_waves, v_waves, out_on_device != 0, nullptr,
                          nullptr, /*solo=*/false, &ev);
    });
}

int vr_evaluate_wave(vr_handle h, const float* mix, const float* inst, int on_device, int64_t L, int tta, int batchsize, int cropsize,
                     int64_t window, double* sums, float* y_wave, float* v_wave, int out_on_device) {
    if (!mix || !inst || !sums) { g_err = "null argument"; return VR_ERR_BAD_ARGUMENT; }
    if (!evaluate_args_ok(1, &mix, &inst, &L, window, &sums, y_wave, v_wave)) return VR_ERR_BAD_ARGUMENT;
    if (L < 1) { g_err = "wave shorter than one hop"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    return guard([&] {
        const long long len = L;
        const vr::EvalArgs ev{&inst, (long long)window, &sums, y_wave != nullptr};
        h->m.separate_run(1, &mix, on_device != 0, nullptr, &len, tta, batchsize, cropsize, &y_wave, &v_wave, out_on_device != 0, nullptr, nullptr,
                          /*solo=*/true, &ev);
    });
}

int vr_evaluate_plan(int hop, int64_t L, int64_t window, int64_t* samples, int64_t* n_windows) {
    return guard([&] {
        const vr::EvalPlan p = vr::evaluate_plan(hop, L, window);
        if (samples) *samples = p.samples;
        if (n_windows) *n_windows = p.windows;
    });
}

// ---- pseudo-instrument labels ---------------------------------------------------------------------------------
// What can be judged without the handle: the count, the tables, the layout.  Everything per song (a null entry, T <= 0, L < hop) and
// training mode need the handle: Model::separate_run refuses them before it touches the device.
static bool pseudo_args_ok(int n_songs, const void* mix, const void* inst, const void* len, const void* out, int layout) {
    if (n_songs <= 0) { g_err = "n_songs must be positive"; return false; }
    if (!mix || !inst || !len || !out) { g_err = "null table"; return false; }
    if (layout != VR_PSEUDO_SPEC && layout != VR_PSEUDO_ROWS) { g_err = "unknown layout (VR_PSEUDO_SPEC or VR_PSEUDO_ROWS)"; return false; }
    return true;
}

int vr_pseudo_many(vr_handle h, int n_songs, const float* const* mix_specs, const float* const* inst_specs, int on_device, const int* T, int tta,
                   int batchsize, int cropsize, int layout, float* const* out, int out_on_device) {
    if (!pseudo_args_ok(n_songs, mix_specs, inst_specs, T, out, layout)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        const vr::PseudoArgs ps{inst_specs, layout};
        h->m.separate_run(n_songs, mix_specs, on_device != 0, T, nullptr, tta, batchsize, cropsize, out, nullptr, out_on_device != 0, nullptr, nullptr,
                          /*solo=*/false, nullptr, &ps);
    });
}

int vr_pseudo_wave_many(vr_handle h, int n_songs, const float* const* mix_waves, const float* const* inst_waves, int on_device, const int64_t* L,
                        int tta, int batchsize, int cropsize, int layout, float* const* out, int out_on_device) {
    if (!pseudo_args_ok(n_songs, mix_waves, inst_waves, L, out, layout)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        std::vector<long long> len(L, L + n_songs);
        const vr::PseudoArgs ps{inst_waves, layout};
        h->m.separate_run(n_songs, mix_waves, on_device != 0, nullptr, len.data(), tta, batchsize, cropsize, out, nullptr, out_on_device != 0, nullptr,
                          nullptr, /*solo=*/false, nullptr, &ps);
    });
}

int vr_pseudo(vr_handle h, const float* mix_spec, const float* inst_spec, int on_device, int T, int tta, int batchsize, int cropsize, int layout,
              float* out, int out_on_device) {
    if (!mix_spec || !inst_spec || !out) { g_err = "null argument"; return VR_ERR_BAD_ARGUMENT; }
    if (!pseudo_args_ok(1, &mix_spec, &inst_spec, &T, &out, layout)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        const vr::PseudoArgs ps{&inst_spec, layout};
        h->m.separate_run(1, &mix_spec, on_device != 0, &T, nullptr, tta, batchsize, cropsize, &out, nullptr, out_on_device != 0, nullptr, nullptr,
                          /*solo=*/true, nullptr, &ps);
    });
}

int vr_pseudo_wave(vr_handle h, const float* mix_wave, const float* inst_wave, int on_device, int64_t L, int tta, int batchsize, int cropsize,
                   int layout, float* out, int out_on_device) {
    if (!mix_wave || !inst_wave || !out) { g_err = "null argument"; return VR_ERR_BAD_ARGUMENT; }
    if (!pseudo_args_ok(1, &mix_wave, &inst_wave, &L, &out, layout)) return VR_ERR_BAD_ARGUMENT;
    NEED(h);
    return guard([&] {
        const long long len = L;
        const vr::PseudoArgs ps{&inst_wave, layout};
        h->m.separate_run(1, &mix_wave, on_device != 0, nullptr, &len, tta, batchsize, cropsize, &out, nullptr, out_on_device != 0, nullptr, nullptr,
                          /*solo=*/true, nullptr, &ps);
    });
}

// ---- WAV sample bytes in, PCM16 out (csrc/pcm.h; the host converters are pcm_host.cpp) ------------------------------------------
int vr_pcm_available(vr_handle h, int* available) {
    NEED(h);
    return guard([&] {
        VR_CHECK(available, VR_ERR_BAD_ARGUMENT, "null argument");
        *available = h->m.pcm_available() ? 1 : 0;
    });
}

int vr_stft_pcm(vr_handle h, const void* bytes, int on_device, int64_t frames, int channels, int fmt, float* spec, int spec_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(bytes && spec, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.stft_pcm_api(bytes, on_device != 0, frames, channels, fmt, spec, spec_on_device != 0);
    });
}

int vr_istft_pcm16(vr_handle h, const float* spec, int on_device, int T, int16_t* out, int out_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(spec && out, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.istft_pcm16_api(spec, on_device != 0, T, out, out_on_device != 0);
    });
}

int vr_separate_pcm(vr_handle h, const void* bytes, int on_device, int64_t frames, int channels, int fmt, int tta, int batchsize,
                    int cropsize, int16_t* y, int16_t* v, int out_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(bytes && y && v, VR_ERR_BAD_ARGUMENT, "null argument");
        const long long len = frames;
        const float* in = static_cast<const float*>(bytes);
        float *ys = reinterpret_cast<float*>(y), *vs = reinterpret_cast<float*>(v);
        h->m.separate_run(1, &in, on_device != 0, nullptr, &len, tta, batchsize, cropsize, &ys, &vs, out_on_device != 0, &channels, &fmt,
                          /*solo=*/true);
    });
}

int vr_separate_pcm_many(vr_handle h, int n_songs, const void* const* bytes, int on_device, const int64_t* frames, const int* channels,
                         const int* fmt, int tta, int batchsize, int cropsize, int16_t* const* y, int16_t* const* v, int out_on_device) {
    if (!many_args_ok(n_songs, bytes, frames, y, v)) return VR_ERR_BAD_ARGUMENT;
    if (!channels || !fmt) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    return guard([&] {
        std::vector<long long> len(frames, frames + n_songs);
        h->m.separate_run(n_songs, reinterpret_cast<const float* const*>(bytes), on_device != 0, nullptr, len.data(), tta, batchsize,
                          cropsize, reinterpret_cast<float* const*>(y), reinterpret_cast<float* const*>(v), out_on_device != 0, channels, fmt);
    });
}

// ---- streaming separation ----------------------------------------------------------------------------------------------------
struct vr_stream_s {
    vr_model* h;
    vr::StreamState* st;
};

#define NEED_STREAM(s)                                           \
    if (!(s) || !(s)->st) {                                      \
        g_err = "null stream";                                   \
        return VR_ERR_BAD_ARGUMENT;                              \
    }

int vr_stream_plan(int n_fft, int hop, int cropsize, int offset, int tta, int64_t samples_in, int flushed, int64_t* frames_ready,
                   int64_t* crops_ready, int64_t* samples_out) {
    return guard([&] {
        const vr::StreamSchedule p = vr::stream_schedule(n_fft, hop, cropsize, offset, tta != 0, samples_in, flushed != 0);
        if (frames_ready) *frames_ready = p.frames;
        if (crops_ready) { crops_ready[0] = p.crops[0]; crops_ready[1] = p.crops[1]; }
        if (samples_out) *samples_out = p.samples_out;
    });
}

int vr_stream_plan_ex(int n_fft, int hop, int cropsize, int offset, int flags, int64_t samples_in, int flushed, int64_t* frames_ready,
                      int64_t* crops_ready, int64_t* samples_out) {
    return guard([&] {
        VR_CHECK(!(flags & ~15), VR_ERR_BAD_ARGUMENT, "unknown vr_stream_open flag");
        const vr::StreamSchedule p = vr::stream_schedule(n_fft, hop, cropsize, offset, (flags & VR_STREAM_TTA) != 0, samples_in, flushed != 0,
                                                         (flags & VR_STREAM_POSTPROCESS) != 0);
        if (frames_ready) *frames_ready = p.frames;
        if (crops_ready) { crops_ready[0] = p.crops[0]; crops_ready[1] = p.crops[1]; }
        if (samples_out) *samples_out = p.samples_out;
    });
}

int vr_stream_open(vr_handle h, int cropsize, int batchsize, int flags, double coef_re, double coef_im, vr_stream* out) {
    if (!out) { g_err = "null out pointer"; return VR_ERR_BAD_ARGUMENT; }
    *out = nullptr;
    NEED(h);
    return guard([&] {
        vr::StreamState* st = h->m.stream_open(cropsize, batchsize, flags, coef_re, coef_im);
        *out = new vr_stream_s{h, st};
    });
}

int vr_stream_push(vr_stream s, const float* wave, int on_device, int64_t n, float* y, float* v, int out_on_device, int64_t capacity,
                   int64_t* n_out) {
    NEED_STREAM(s);
    return guard([&] {
        long long got = 0;
        s->h->m.stream_push(*s->st, wave, on_device != 0, n, false, y, v, out_on_device != 0, capacity, &got);
        if (n_out) *n_out = got;
    });
}

int vr_stream_flush(vr_stream s, float* y, float* v, int out_on_device, int64_t capacity, int64_t* n_out) {
    NEED_STREAM(s);
    return guard([&] {
        long long got = 0;
        s->h->m.stream_push(*s->st, nullptr, false, 0, true, y, v, out_on_device != 0, capacity, &got);
        if (n_out) *n_out = got;
    });
}

int vr_stream_push_many(int n_streams, const vr_stream* s, const float* const* wave, int on_device, const int64_t* n, const int* flush,
                        int batchsize, float* const* y, float* const* v, int out_on_device, const int64_t* capacity, int64_t* n_out) {
    if (n_streams <= 0) { g_err = "n_streams must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (!s || !n) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        std::vector<vr::StreamState*> st((size_t)n_streams);
        std::vector<long long> len(n, n + n_streams), cap, got((size_t)n_streams, 0);
        if (capacity) cap.assign(capacity, capacity + n_streams);
        for (int k = 0; k < n_streams; ++k) {
            const std::string who = "stream " + std::to_string(k) + ": ";
            VR_CHECK(s[k] && s[k]->st, VR_ERR_BAD_ARGUMENT, who + "null stream (closed?)");
            VR_CHECK(s[k]->h == s[0]->h, VR_ERR_BAD_ARGUMENT, who + "belongs to another handle than stream 0: the streams of one call share a handle");
            st[k] = s[k]->st;
        }
        s[0]->h->m.stream_push_many(n_streams, st.data(), wave, on_device != 0, len.data(), flush, batchsize, y, v, out_on_device != 0,
                                    capacity ? cap.data() : nullptr, got.data());
        if (n_out) for (int k = 0; k < n_streams; ++k) n_out[k] = got[k];
    });
}

// The argument checks of the *_push_pcm entry points that need neither a device nor the stream or session: format, channel count (streams:
// 1 or 2; sessions: positive here, the session's or 1 once it is known), frame count, a null buffer.  `who` in front of the message.
static void check_pcm_args(const std::string& who, const void* bytes, int64_t frames, int channels, int fmt, bool stream) {
    VR_CHECK(fmt == VR_PCM_S16 || fmt == VR_PCM_S24 || fmt == VR_PCM_S32 || fmt == VR_PCM_F32, VR_ERR_BAD_ARGUMENT,
             who + "unknown sample format " + std::to_string(fmt) + " (VR_PCM_S16 / S24 / S32 / F32)");
    if (stream) VR_CHECK(channels == 1 || channels == 2, VR_ERR_BAD_ARGUMENT, who + "1 or 2 channels, not " + std::to_string(channels));
    else VR_CHECK(channels >= 1, VR_ERR_BAD_ARGUMENT, who + "frames of " + std::to_string(channels) + " channels: a block holds the session's or 1");
    VR_CHECK(frames >= 0, VR_ERR_BAD_ARGUMENT, who + "negative frame count");
    VR_CHECK(frames == 0 || bytes, VR_ERR_BAD_ARGUMENT, who + "null input");
}

int vr_stream_push_pcm(vr_stream s, const void* bytes, int on_device, int64_t frames, int channels, int fmt, float* y, float* v,
                       int out_on_device, int64_t capacity, int64_t* n_out) {
    const int rc = guard([&] { check_pcm_args("", bytes, frames, channels, fmt, true); });
    if (rc != VR_OK) return rc;
    NEED_STREAM(s);
    return guard([&] {
        long long got = 0;
        s->h->m.stream_push(*s->st, static_cast<const float*>(bytes), on_device != 0, frames, false, y, v, out_on_device != 0, capacity, &got,
                            channels, fmt);
        if (n_out) *n_out = got;
    });
}

int vr_stream_push_many_pcm(int n_streams, const vr_stream* s, const void* const* bytes, int on_device, const int64_t* frames,
                            const int* channels, const int* fmt, const int* flush, int batchsize, float* const* y, float* const* v,
                            int out_on_device, const int64_t* capacity, int64_t* n_out) {
    if (n_streams <= 0) { g_err = "n_streams must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (!s || !frames || !channels || !fmt) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        for (int k = 0; k < n_streams; ++k)
            check_pcm_args("stream " + std::to_string(k) + ": ", bytes ? bytes[k] : nullptr, frames[k], channels[k], fmt[k], true);
        std::vector<vr::StreamState*> st((size_t)n_streams);
        std::vector<long long> len(frames, frames + n_streams), cap, got((size_t)n_streams, 0);
        if (capacity) cap.assign(capacity, capacity + n_streams);
        for (int k = 0; k < n_streams; ++k) {
            const std::string who = "stream " + std::to_string(k) + ": ";
            VR_CHECK(s[k] && s[k]->st, VR_ERR_BAD_ARGUMENT, who + "null stream (closed?)");
            VR_CHECK(s[k]->h == s[0]->h, VR_ERR_BAD_ARGUMENT, who + "belongs to another handle than stream 0: the streams of one call share a handle");
            st[k] = s[k]->st;
        }
        s[0]->h->m.stream_push_many(n_streams, st.data(), reinterpret_cast<const float* const*>(bytes), on_device != 0, len.data(), flush, batchsize,
                                    y, v, out_on_device != 0, capacity ? cap.data() : nullptr, got.data(), channels, fmt);
        if (n_out) for (int k = 0; k < n_streams; ++k) n_out[k] = got[k];
    });
}

int vr_stream_coef(vr_stream s, double* coef_re_im) {
    NEED_STREAM(s);
    return guard([&] {
        VR_CHECK(coef_re_im, VR_ERR_BAD_ARGUMENT, "null argument");
        VR_CHECK(s->st->measure && s->st->flushed, VR_ERR_BAD_ARGUMENT, "vr_stream_coef: the normaliser exists after the flush of a VR_STREAM_MEASURE stream");
        coef_re_im[0] = s->st->coef[0];
        coef_re_im[1] = s->st->coef[1];
    });
}

int vr_stream_info(vr_stream s, int64_t* lookahead_samples, int64_t* block_samples, int64_t* state_bytes) {
    NEED_STREAM(s);
    return guard([&] {
        const vr::Model& m = s->h->m;
        if (lookahead_samples) *lookahead_samples = (int64_t)(s->st->roi + m.offset + (s->st->post ? vr::kStreamPostDelay : 0)) * m.hop;
        if (block_samples) *block_samples = (int64_t)s->st->roi * m.hop;
        if (state_bytes) *state_bytes = (int64_t)s->st->state_bytes;
    });
}

int vr_stream_close(vr_stream s) {
    if (!s) { g_err = "null stream"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        s->h->m.stream_close(s->st);
        delete s;
    });
}

int vr_arena_bytes(vr_handle h, int64_t* staging_bytes, int64_t* workspace_bytes) {
    NEED(h);
    return guard([&] {
        long long a = 0, b = 0;
        h->m.arena_bytes(&a, &b);
        if (staging_bytes) *staging_bytes = a;
        if (workspace_bytes) *workspace_bytes = b;
    });
}

int vr_pipeline_buffer(vr_handle h, int64_t* bytes, int release) {
    NEED(h);
    return guard([&] {
        const long long held = h->m.pipeline_buffer(release != 0);
        if (bytes) *bytes = held;
    });
}

int vr_train_step(vr_handle h, const float* X, const float* y, int on_device, int B, int T, int accumulation_steps,
                  float* loss_out, float* mask_out, int mask_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(X && y, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.need_real_mask("vr_train_step");
        h->m.train_fwd_bwd_api(X, y, on_device != 0, B, T, accumulation_steps, loss_out, mask_out, mask_on_device != 0);
    });
}

int vr_forward_train(vr_handle h, const float* X, int on_device, int B, int T, float* mask_out, int mask_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(X && mask_out, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.need_real_mask("vr_forward_train");
        h->m.forward_train_api(X, on_device != 0, B, T, mask_out, mask_on_device != 0);
    });
}

int vr_backward(vr_handle h, const float* dmask, int on_device) {
    NEED(h);
    return guard([&] {
        h->m.need_real_mask("vr_backward");
        h->m.backward_api(dmask, on_device != 0);
    });
}

int vr_graph_generation(vr_handle h, int64_t* generation, int* valid) {
    NEED(h);
    return guard([&] {
        VR_CHECK(generation, VR_ERR_BAD_ARGUMENT, "null argument");
        *generation = h->m.graph_gen;
        if (valid) *valid = h->m.graph_valid ? 1 : 0;
    });
}

int vr_param_arena(vr_handle h, float** device_ptr, int64_t* numel) {
    NEED(h);
    return guard([&] {
        VR_CHECK(device_ptr && numel, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.param_arena(device_ptr, numel);
    });
}

// ex: desc is a table of vr_aug_ex, the _ex entry points (a remix partner's crops lie where a mixup partner's do)
static int augment_batch(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const void* desc,
                         const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_mag, float* y_mag,
                         int out_on_device, bool out_complex, bool ex = false) {
    static_assert(sizeof(vr_aug_ex) == sizeof(vr::AugDescEx) && offsetof(vr_aug_ex, gain_y) == offsetof(vr::AugDescEx, gain_y) &&
                      offsetof(vr_aug_ex, gain_v) == offsetof(vr::AugDescEx, gain_v) && sizeof(vr_aug_ex) == 24,
                  "C ABI struct and its kernels.h twin");
    static_assert(VR_AUG_REMIX == vr::kAugRemix && VR_AUG_MONO == vr::kAugMono && VR_AUG_MIX_MONO == vr::kAugMixMono && VR_AUG_MIXUP == vr::kAugMix,
                  "flag bits of the header and of kernels.h");
    NEED(h);
    return guard([&] {
        VR_CHECK(X && y && desc && X_mag && y_mag, VR_ERR_BAD_ARGUMENT, "null argument");
        bool mix = false, red = false;
        for (int b = 0; b < B; ++b) {
            const int flags = ex ? static_cast<const vr_aug_ex*>(desc)[b].flags : static_cast<const vr_aug*>(desc)[b].flags;
            mix = mix || (flags & (ex ? 8 | VR_AUG_REMIX : 8));
            red = red || (flags & (1 | 16));
        }
        VR_CHECK(!mix || (X_mix && y_mix), VR_ERR_BAD_ARGUMENT, ex ? "mixup or remix flagged but no partner crops given" : "mixup flagged but no partner crops given");
        VR_CHECK(!red || reduction_weight, VR_ERR_BAD_ARGUMENT, "vocal reduction flagged but no reduction_weight given");
        h->m.augment_api(X, y, X_mix, y_mix, desc, reduction_weight, B, T, bins, in_on_device != 0, X_mag, y_mag,
                         out_on_device != 0, out_complex, ex);
    });
}

// ---- the resident training set ---------------------------------------------------------------------------------------------
static void need_device(int device);

struct vr_dataset_s {
    vr::ResidentSet set;
    vr_dataset_s(int device, int bins) : set(device, bins) {}
    vr_dataset_s(int device, int n_fft, int hop) : set(device, n_fft, hop) {}
};

#define NEED_DATASET(d)                                          \
    if (!(d)) {                                                  \
        g_err = "null dataset";                                  \
        return VR_ERR_BAD_ARGUMENT;                              \
    }

int vr_dataset_create(int device, int bins, vr_dataset* out) {
    if (!out) { g_err = "null out pointer"; return VR_ERR_BAD_ARGUMENT; }
    *out = nullptr;
    if (bins <= 0) { g_err = "vr_dataset_create: bins must be positive"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        need_device(device);
        *out = new vr_dataset_s(device, bins);
    });
}

// The wave store: the sizes are judged on the host alone (stft_crops_supported), so an unsupported pair is refused without a device.
int vr_dataset_create_waves(int device, int n_fft, int hop_length, vr_dataset* out) {
    if (!out) { g_err = "null out pointer"; return VR_ERR_BAD_ARGUMENT; }
    *out = nullptr;
    if (n_fft <= 0 || hop_length <= 0) { g_err = "vr_dataset_create_waves: n_fft and hop_length must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (hop_length * 2 != n_fft || !vr::stft_crops_supported(n_fft, hop_length)) {
        g_err = "vr_dataset_create_waves: n_fft " + std::to_string(n_fft) + ", hop_length " + std::to_string(hop_length) +
                ": the wave store forms its rows with the frame-tiled STFT, which needs hop_length == n_fft / 2 and a power-of-two n_fft "
                "from 128 up to what its tile holds in LDS; keep such a set as cached rows (vr_dataset_create)";
        return VR_ERR_UNSUPPORTED;
    }
    return guard([&] {
        need_device(device);
        *out = new vr_dataset_s(device, n_fft, hop_length);
    });
}

int vr_dataset_add_waves(vr_dataset d, const float* mix, const float* inst, int on_device, int64_t n, int* song_out) {
    NEED_DATASET(d);
    return guard([&] {
        VR_CHECK(mix && inst, VR_ERR_BAD_ARGUMENT, "null argument");
        const int song = d->set.add_waves(mix, inst, on_device != 0, n);
        if (song_out) *song_out = song;
    });
}

int vr_dataset_add_pcm(vr_dataset d, const void* mix_bytes, const void* inst_bytes, int on_device, int64_t frames, int mix_channels,
                       int inst_channels, int mix_fmt, int inst_fmt, int* song_out) {
    NEED_DATASET(d);
    return guard([&] {
        VR_CHECK(mix_bytes && inst_bytes, VR_ERR_BAD_ARGUMENT, "null argument");
        const int channels[2] = {mix_channels, inst_channels}, fmt[2] = {mix_fmt, inst_fmt};
        const int song = d->set.add_pcm(mix_bytes, inst_bytes, on_device != 0, frames, channels, fmt);
        if (song_out) *song_out = song;
    });
}

int vr_dataset_destroy(vr_dataset d) {
    NEED_DATASET(d);
    return guard([&] { delete d; });
}

int vr_dataset_add(vr_dataset d, const float* X, const float* y, int64_t rows, int* song_out) {
    NEED_DATASET(d);
    return guard([&] {
        VR_CHECK(X && y, VR_ERR_BAD_ARGUMENT, "null argument");
        const int song = d->set.add(X, y, rows);
        if (song_out) *song_out = song;
    });
}

int vr_dataset_info(vr_dataset d, int* n_songs, int64_t* bytes) {
    NEED_DATASET(d);
    if (n_songs) *n_songs = (int)d->set.songs.size();
    if (bytes) *bytes = d->set.bytes;
    return VR_OK;
}

int vr_dataset_rows(vr_dataset d, int song, int64_t* rows) {
    NEED_DATASET(d);
    return guard([&] {
        VR_CHECK(rows, VR_ERR_BAD_ARGUMENT, "null argument");
        VR_CHECK(song >= 0 && song < (int)d->set.songs.size(), VR_ERR_BAD_ARGUMENT,
                 "vr_dataset_rows: song " + std::to_string(song) + " out of range (the dataset holds " + std::to_string(d->set.songs.size()) + ")");
        *rows = d->set.songs[song].rows;
    });
}

int vr_dataset_peak(vr_dataset d, int song, float* peak, float* at, int* slab, int64_t* index) {
    NEED_DATASET(d);
    if (!peak) { g_err = "null argument"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        long long idx = 0;
        *peak = d->set.peak(song, at, slab, &idx);
        if (index) *index = idx;
    });
}

int vr_augment_batch(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug* desc,
                     const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_mag, float* y_mag,
                     int out_on_device) {
    return augment_batch(h, X, y, X_mix, y_mix, desc, reduction_weight, B, T, bins, in_on_device, X_mag, y_mag, out_on_device, false);
}

int vr_augment_batch_complex(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug* desc,
                             const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_out, float* y_out,
                             int out_on_device) {
    return augment_batch(h, X, y, X_mix, y_mix, desc, reduction_weight, B, T, bins, in_on_device, X_out, y_out, out_on_device, true);
}

int vr_augment_batch_ex(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug_ex* desc,
                        const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_mag, float* y_mag,
                        int out_on_device) {
    return augment_batch(h, X, y, X_mix, y_mix, desc, reduction_weight, B, T, bins, in_on_device, X_mag, y_mag, out_on_device, false, true);
}

int vr_augment_batch_complex_ex(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug_ex* desc,
                                const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_out, float* y_out,
                                int out_on_device) {
    return augment_batch(h, X, y, X_mix, y_mix, desc, reduction_weight, B, T, bins, in_on_device, X_out, y_out, out_on_device, true, true);
}

// The tables and the batch size are checked before the handle and the store, so that a caller's argument error is reported without a
// device (as vr_separate_many does).
static int dataset_batch(vr_handle h, vr_dataset d, const vr_crop* crops, const void* desc, const float* reduction_weight, int B, int T,
                         float* X_mag, float* y_mag, int out_on_device, bool out_complex, bool ex = false) {
    if (B <= 0) { g_err = "B must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (!crops || !desc || !X_mag || !y_mag) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    NEED_DATASET(d);
    static_assert(sizeof(vr_crop) == sizeof(vr::ResidentCrop) && sizeof(vr_aug) == sizeof(vr::AugDesc), "C ABI structs and their kernels.h twins");
    return guard([&] {
        h->m.dataset_batch_api(d->set, reinterpret_cast<const vr::ResidentCrop*>(crops), desc, reduction_weight, B, T, X_mag, y_mag,
                               out_on_device != 0, out_complex, ex);
    });
}

int vr_dataset_batch_ex(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug_ex* desc, const float* reduction_weight, int B, int T,
                        float* X_mag, float* y_mag, int out_on_device) {
    return dataset_batch(h, d, crops, desc, reduction_weight, B, T, X_mag, y_mag, out_on_device, false, true);
}

int vr_dataset_batch_complex_ex(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug_ex* desc, const float* reduction_weight, int B,
                                int T, float* X_out, float* y_out, int out_on_device) {
    return dataset_batch(h, d, crops, desc, reduction_weight, B, T, X_out, y_out, out_on_device, true, true);
}

int vr_dataset_batch(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug* desc, const float* reduction_weight, int B, int T,
                     float* X_mag, float* y_mag, int out_on_device) {
    return dataset_batch(h, d, crops, desc, reduction_weight, B, T, X_mag, y_mag, out_on_device, false);
}

int vr_dataset_batch_complex(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug* desc, const float* reduction_weight, int B, int T,
                             float* X_out, float* y_out, int out_on_device) {
    return dataset_batch(h, d, crops, desc, reduction_weight, B, T, X_out, y_out, out_on_device, true);
}

// (argument errors first, as dataset_batch)
static int dataset_windows(vr_handle h, vr_dataset d, const vr_window* w, int B, int T, float* X_out, float* y_out, int out_on_device,
                           bool out_complex) {
    if (B <= 0) { g_err = "B must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (!w || !X_out || !y_out) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    NEED_DATASET(d);
    static_assert(sizeof(vr_window) == sizeof(vr::ResidentWindow) && offsetof(vr_window, scale) == offsetof(vr::ResidentWindow, scale),
                  "C ABI struct and its model.h twin");
    return guard([&] {
        h->m.dataset_windows_api(d->set, reinterpret_cast<const vr::ResidentWindow*>(w), B, T, X_out, y_out, out_on_device != 0, out_complex);
    });
}

int vr_dataset_windows(vr_handle h, vr_dataset d, const vr_window* w, int B, int T, float* X_mag, float* y_mag, int out_on_device) {
    return dataset_windows(h, d, w, B, T, X_mag, y_mag, out_on_device, false);
}

int vr_dataset_windows_complex(vr_handle h, vr_dataset d, const vr_window* w, int B, int T, float* X_out, float* y_out, int out_on_device) {
    return dataset_windows(h, d, w, B, T, X_out, y_out, out_on_device, true);
}

int vr_adam_step(vr_handle h, double lr, double b1, double b2, double eps, double grad_scale) {
    NEED(h);
    return guard([&] { h->m.adam_step_api(lr, b1, b2, eps, grad_scale); });
}

int vr_get_adam_state(vr_handle h, float* exp_avg, float* exp_avg_sq, int64_t numel, int64_t* step) {
    NEED(h);
    return guard([&] {
        VR_CHECK(exp_avg && exp_avg_sq && step, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.adam_state(exp_avg, exp_avg_sq, numel, step, false);
    });
}

int vr_set_adam_state(vr_handle h, const float* exp_avg, const float* exp_avg_sq, int64_t numel, int64_t step) {
    NEED(h);
    return guard([&] {
        VR_CHECK(exp_avg && exp_avg_sq, VR_ERR_BAD_ARGUMENT, "null argument");
        int64_t st = step;
        h->m.adam_state(const_cast<float*>(exp_avg), const_cast<float*>(exp_avg_sq), numel, &st, true);
    });
}

int vr_zero_grad(vr_handle h) {
    NEED(h);
    return guard([&] { h->m.zero_grad_api(); });
}

int vr_get_grad(vr_handle h, const char* key, float* host, int64_t capacity_bytes) {
    NEED(h);
    return guard([&] {
        VR_CHECK(key && host, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.get_grad(key, host, capacity_bytes);
    });
}

int vr_set_dropout(vr_handle h, int mode, uint64_t seed, const float* masks, int B) {
    NEED(h);
    return guard([&] { h->m.set_dropout(mode, seed, masks, B); });
}

int vr_grad_arena(vr_handle h, float** device_ptr, int64_t* numel) {
    NEED(h);
    return guard([&] {
        VR_CHECK(device_ptr && numel, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.grad_arena(device_ptr, numel);
    });
}

int vr_validate_step(vr_handle h, const float* X, const float* y, int on_device, int B, int T, float* loss_out) {
    NEED(h);
    return guard([&] {
        VR_CHECK(X && y, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.validate_api(X, y, on_device != 0, B, T, loss_out);
    });
}

int vr_comm_unique_id(void* id_out) {
    return guard([&] {
        VR_CHECK(id_out, VR_ERR_BAD_ARGUMENT, "null argument");
        vr::comm_unique_id(id_out);
    });
}

int vr_comm_init(vr_handle h, int rank, int world_size, const void* id) {
    NEED(h);
    return guard([&] { h->m.comm_init(rank, world_size, id); });
}

int vr_comm_destroy(vr_handle h) {
    NEED(h);
    return guard([&] { h->m.comm_destroy(); });
}

int vr_allreduce_grads(vr_handle h, int wire_dtype) {
    NEED(h);
    return guard([&] { h->m.allreduce_grads(wire_dtype); });
}

int vr_broadcast_params(vr_handle h, int root, int with_optimizer) {
    NEED(h);
    return guard([&] { h->m.broadcast_params(root, with_optimizer != 0); });
}

int vr_debug_kernel(vr_handle h, const char* name, const int64_t* dims, int ndims, const float* fparams, int nfparams,
                    const float* const* inputs, int ninputs, float* const* outputs, int noutputs) {
    NEED(h);
    return guard([&] {
        VR_CHECK(name && dims && inputs && outputs, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.debug_kernel(name, dims, ndims, fparams, nfparams, inputs, ninputs, outputs, noutputs);
    });
}

static void need_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw vr::Error(VR_ERR_HIP, "no HIP device visible: libvr_mi355 has no CPU fallback");
    if (device < 0 || device >= count) throw vr::Error(VR_ERR_BAD_ARGUMENT, "device index out of range");
}

int vr_resample(int device, const float* x, int channels, int64_t n_in, int sr_in, int sr_out, float* y, int64_t n_out) {
    return guard([&] {
        VR_CHECK(x && y, VR_ERR_BAD_ARGUMENT, "null argument");
        need_device(device);
        vr::resample_api(device, x, channels, n_in, sr_in, sr_out, y, n_out);
    });
}

int vr_resample_ratio(int device, const float* x, int channels, int64_t n_in, double ratio, float* y, int64_t n_out) {
    return guard([&] {
        VR_CHECK(x && y, VR_ERR_BAD_ARGUMENT, "null argument");
        need_device(device);
        vr::resample_ratio_api(device, x, channels, n_in, ratio, y, n_out);
    });
}

// ---- pitch-shifted waves and training pairs (csrc/pitch.hip) --------------------------------------------------------------------
int vr_pitch_plan(int64_t L, int n_fft, int hop, double rate, double ratio, int* T, int* T_stretch, int64_t* n_stretch, int64_t* n_resampled) {
    return guard([&] {
        const vr::PitchPlan p = vr::pitch_plan(L, n_fft, hop, rate, ratio);
        if (T) *T = p.T;
        if (T_stretch) *T_stretch = p.T_stretch;
        if (n_stretch) *n_stretch = p.n_stretch;
        if (n_resampled) *n_resampled = p.n_resampled;
    });
}

int vr_phase_vocoder(vr_handle h, const float* spec, int on_device, int signals, int T, double rate, float* out, int out_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(spec && out, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.phase_vocoder_api(spec, on_device != 0, signals, T, rate, out, out_on_device != 0);
    });
}

int vr_istft_length(vr_handle h, const float* spec, int spec_on_device, int T, int64_t length, float* wave, int wave_on_device) {
    NEED(h);
    return guard([&] {
        VR_CHECK(spec && wave, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.istft_length_api(spec, spec_on_device != 0, T, length, wave, wave_on_device != 0);
    });
}

int vr_pitch_shift_many(vr_handle h, int n, const float* const* waves, int on_device, int channels, const int64_t* L, double rate, double ratio,
                        int64_t max_bytes, float* const* out, int out_on_device) {
    if (n <= 0 || !waves || !L || !out) { g_err = "pitch shift: no item or a null table"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    return guard([&] {
        std::vector<long long> len(L, L + n);
        h->m.pitch_run(n, waves, nullptr, on_device != 0, channels, len.data(), h->m.n_fft, h->m.hop, rate, ratio, max_bytes, out, nullptr, nullptr,
                       0, out_on_device != 0);
    });
}

int vr_pitch_pair_many(vr_handle h, int n, const float* const* mix, const float* const* inst, int on_device, const int64_t* L, int shift_n_fft,
                       int shift_hop, double rate, double ratio, int layout, int64_t max_bytes, float* const* X_out, float* const* y_out,
                       int out_on_device) {
    if (n <= 0 || !mix || !inst || !L || !X_out || !y_out) { g_err = "pitch pair: no item or a null table"; return VR_ERR_BAD_ARGUMENT; }
    NEED(h);
    return guard([&] {
        std::vector<long long> len(L, L + n);
        h->m.pitch_run(n, mix, inst, on_device != 0, 2, len.data(), shift_n_fft, shift_hop, rate, ratio, max_bytes, nullptr, X_out, y_out, layout,
                       out_on_device != 0);
    });
}

// ---- plain training pairs: trim, align, STFT rows and peak (csrc/prepare.hip) ------------------------------------------------------
static_assert(sizeof(vr_pair_window) == sizeof(vr::PairWindow) && offsetof(vr_pair_window, n) == offsetof(vr::PairWindow, n),
              "vr_pair_window and vr::PairWindow must agree");

int vr_pair_window_plan(int64_t a_start, int64_t a_end, int64_t b_start, int64_t b_end, int64_t lag, vr_pair_window* out) {
    return guard([&] {
        VR_CHECK(out, VR_ERR_BAD_ARGUMENT, "null argument");
        VR_CHECK(a_start >= 0 && a_start <= a_end && b_start >= 0 && b_start <= b_end, VR_ERR_BAD_ARGUMENT,
                 "pair window: a trimmed range must be 0 <= start <= end");
        vr::PairWindow w{a_start, a_end, b_start, b_end, lag, 0, 0, 0};
        const bool ok = vr::pair_window_plan(w);
        std::memcpy(out, &w, sizeof(w));
        VR_CHECK(ok, VR_ERR_BAD_ARGUMENT, "pair window: the common window is empty (n = " + std::to_string(w.n) + ")");
    });
}

int vr_align_pair_many(int device, int n, const float* const* mix, const float* const* inst, int on_device, const int64_t* L_mix,
                       const int64_t* L_inst, int sr, vr_pair_window* out) {
    if (n <= 0 || !mix || !inst || !L_mix || !L_inst || !out) { g_err = "align pair: no pair or a null table"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        std::vector<long long> la(L_mix, L_mix + n), lb(L_inst, L_inst + n);
        vr::align_pair_check(n, mix, inst, la.data(), lb.data(), sr, out);
        need_device(device);
        vr::align_pair_many_api(device, n, mix, inst, on_device != 0, la.data(), lb.data(), sr, reinterpret_cast<vr::PairWindow*>(out));
    });
}

int vr_pair_rows_many(vr_handle h, int n, const float* const* mix, const float* const* inst, int on_device, const int64_t* L_mix,
                      const int64_t* L_inst, const vr_pair_window* w, int64_t max_bytes, float* const* X_out, float* const* y_out,
                      int out_on_device, float* peaks) {
    if (n <= 0 || !mix || !inst || !L_mix || !L_inst || !w || !X_out || !y_out || !peaks) {
        g_err = "pair rows: no pair or a null table";
        return VR_ERR_BAD_ARGUMENT;
    }
    NEED(h);
    return guard([&] {
        std::vector<long long> la(L_mix, L_mix + n), lb(L_inst, L_inst + n);
        h->m.pair_rows_run(n, mix, inst, on_device != 0, la.data(), lb.data(), reinterpret_cast<const vr::PairWindow*>(w), max_bytes, X_out, y_out,
                           out_on_device != 0, peaks);
    });
}

// ---- the streamed resampler --------------------------------------------------------------------------------------------------
struct vr_resampler_s {
    vr::Resampler* r;
};

#define NEED_RESAMPLER(r)                                        \
    if (!(r) || !(r)->r) {                                       \
        g_err = "null resampler";                                \
        return VR_ERR_BAD_ARGUMENT;                              \
    }

int vr_resampler_plan(int sr_in, int sr_out, int64_t samples_in, int flushed, int64_t* samples_out) {
    return guard([&] {
        const long long out = vr::resampler_plan(sr_in, sr_out, samples_in, flushed != 0);
        if (samples_out) *samples_out = out;
    });
}

int vr_resampler_open(int device, int channels, int sr_in, int sr_out, vr_resampler* out) {
    if (!out) { g_err = "null out pointer"; return VR_ERR_BAD_ARGUMENT; }
    *out = nullptr;
    return guard([&] {
        VR_CHECK(channels > 0 && channels <= 65535, VR_ERR_BAD_ARGUMENT, "resampler: channels must be positive (and at most 65535, one grid row each)");
        vr::resampler_plan(sr_in, sr_out, 0, false);                  // the rate checks, before the device is looked at
        need_device(device);
        *out = new vr_resampler_s{vr::resampler_open(device, channels, sr_in, sr_out)};
    });
}

static int resampler_push_one(vr_resampler r, const float* x, int x_on_device, int64_t n, int flush, float* y, int y_on_device,
                              int64_t capacity, int64_t* n_out) {
    NEED_RESAMPLER(r);
    return guard([&] {
        const long long len = n, cap = capacity;
        long long got = 0;
        vr::resampler_push_many(1, &r->r, &x, x_on_device != 0, &len, &flush, &y, y_on_device != 0, &cap, &got, false);
        if (n_out) *n_out = got;
    });
}

int vr_resampler_push(vr_resampler r, const float* x, int x_on_device, int64_t n, float* y, int y_on_device, int64_t capacity,
                      int64_t* n_out) {
    return resampler_push_one(r, x, x_on_device, n, 0, y, y_on_device, capacity, n_out);
}

int vr_resampler_flush(vr_resampler r, float* y, int y_on_device, int64_t capacity, int64_t* n_out) {
    return resampler_push_one(r, nullptr, 0, 0, 1, y, y_on_device, capacity, n_out);
}

int vr_resampler_push_many(int n, const vr_resampler* r, const float* const* x, int on_device, const int64_t* n_in, const int* flush,
                           float* const* y, int y_on_device, const int64_t* capacity, int64_t* n_out) {
    if (n <= 0) { g_err = "n must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (!r || !n_in) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        std::vector<vr::Resampler*> rs((size_t)n);
        std::vector<long long> len(n_in, n_in + n), cap, got((size_t)n, 0);
        if (capacity) cap.assign(capacity, capacity + n);
        for (int k = 0; k < n; ++k) rs[k] = r[k] ? r[k]->r : nullptr;
        vr::resampler_push_many(n, rs.data(), x, on_device != 0, len.data(), flush, y, y_on_device != 0, capacity ? cap.data() : nullptr,
                                got.data(), true);
        if (n_out) for (int k = 0; k < n; ++k) n_out[k] = got[k];
    });
}

int vr_resampler_push_pcm(vr_resampler r, const void* bytes, int on_device, int64_t frames, int channels, int fmt, float* y, int y_on_device,
                          int64_t capacity, int64_t* n_out) {
    const int rc = guard([&] { check_pcm_args("resampler: ", bytes, frames, channels, fmt, false); });
    if (rc != VR_OK) return rc;
    NEED_RESAMPLER(r);
    return guard([&] {
        long long len = frames, cap = capacity, got = 0;
        const int no_flush = 0;
        vr::resampler_push_many(1, &r->r, nullptr, on_device != 0, &len, &no_flush, &y, y_on_device != 0, &cap, &got, false, &bytes, &channels, &fmt);
        if (n_out) *n_out = got;
    });
}

int vr_resampler_push_many_pcm(int n, const vr_resampler* r, const void* const* bytes, int on_device, const int64_t* frames, const int* channels,
                               const int* fmt, const int* flush, float* const* y, int y_on_device, const int64_t* capacity, int64_t* n_out) {
    if (n <= 0) { g_err = "n must be positive"; return VR_ERR_BAD_ARGUMENT; }
    if (!r || !frames || !channels || !fmt) { g_err = "null table"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        for (int k = 0; k < n; ++k)
            check_pcm_args("resampler " + std::to_string(k) + ": ", bytes ? bytes[k] : nullptr, frames[k], channels[k], fmt[k], false);
        std::vector<vr::Resampler*> rs((size_t)n);
        std::vector<long long> len(frames, frames + n), cap, got((size_t)n, 0);
        if (capacity) cap.assign(capacity, capacity + n);
        for (int k = 0; k < n; ++k) rs[k] = r[k] ? r[k]->r : nullptr;
        vr::resampler_push_many(n, rs.data(), nullptr, on_device != 0, len.data(), flush, y, y_on_device != 0, capacity ? cap.data() : nullptr,
                                got.data(), true, bytes, channels, fmt);
        if (n_out) for (int k = 0; k < n; ++k) n_out[k] = got[k];
    });
}

int vr_resampler_info(vr_resampler r, int64_t* lookahead_samples, int64_t* state_bytes) {
    NEED_RESAMPLER(r);
    return guard([&] {
        long long a = 0, b = 0;
        vr::resampler_info(r->r, &a, &b);
        if (lookahead_samples) *lookahead_samples = a;
        if (state_bytes) *state_bytes = b;
    });
}

int vr_resampler_close(vr_resampler r) {
    if (!r) { g_err = "null resampler"; return VR_ERR_BAD_ARGUMENT; }
    return guard([&] {
        if (r->r) vr::resampler_close(r->r);
        delete r;
    });
}

int vr_xcorr_argmax(int device, const float* a, int64_t na, const float* b, int64_t nb, int64_t* argmax_out) {
    return guard([&] {
        VR_CHECK(a && b && argmax_out, VR_ERR_BAD_ARGUMENT, "null argument");
        need_device(device);
        long long best = 0;
        vr::xcorr_argmax_api(device, a, na, b, nb, &best);
        *argmax_out = best;
    });
}

int vr_profile_begin(vr_handle h) {
    NEED(h);
    return guard([&] { h->m.profile_begin(); });
}

int vr_profile_end(vr_handle h, double* conv_ms, double* conv_flops, int* conv_launches, double* conv_bytes) {
    NEED(h);
    return guard([&] { h->m.profile_end(conv_ms, conv_flops, conv_bytes, conv_launches); });
}

int64_t vr_profile_report(vr_handle h, char* buf, int64_t capacity) {
    if (!h) { g_err = "null handle"; return VR_ERR_BAD_ARGUMENT; }
    const std::string& r = h->m.profile_report;
    if (buf && capacity > 0) {
        const size_t n = std::min<size_t>(r.size(), (size_t)capacity - 1);
        std::memcpy(buf, r.data(), n);
        buf[n] = 0;
    }
    return (int64_t)r.size() + 1;
}

int vr_debug_conv2d(vr_handle h, const float* x, int N, int Cin, int H, int W, const float* w, int Cout, int ksize,
                    int stride, int dil_h, int dil_w, int upsample, const float* affine, float slope, const float* bias,
                    float* out, float* stats_out) {
    NEED(h);
    return guard([&] {
        VR_CHECK(x && w && out, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.debug_conv(x, N, Cin, H, W, w, Cout, ksize, stride, dil_h, dil_w, upsample, affine, slope, bias, out, stats_out);
    });
}

int vr_debug_conv2d_backward(vr_handle h, const float* x, int N, int Cin, int H, int W, const float* w, int Cout,
                             int ksize, int stride, int dil_h, int dil_w, int upsample, const float* affine, float slope,
                             const float* dz, float* dx_out, float* dw_out) {
    NEED(h);
    return guard([&] {
        VR_CHECK(x && w && dz && dx_out && dw_out, VR_ERR_BAD_ARGUMENT, "null argument");
        h->m.debug_conv_bwd(x, N, Cin, H, W, w, Cout, ksize, stride, dil_h, dil_w, upsample, affine, slope, dz, dx_out, dw_out);
    });
}

int vr_debug_merge_artifacts_weight(const float* frame_min, int T, float thres, int min_range, int fade_size,
                                    float* weight_out) {
    return guard([&] {
        VR_CHECK(frame_min && weight_out && T > 0, VR_ERR_BAD_ARGUMENT, "null argument");
        std::vector<float> f(frame_min, frame_min + T), w;
        vr::merge_artifacts_weight(f, w, thres, min_range, fade_size);
        std::memcpy(weight_out, w.data(), (size_t)T * sizeof(float));
    });
}

int vr_debug_stream_post_weight(const float* frame_min, int T, const int* cuts, int n_cuts, float* weight_out, int* final_after_out) {
    return guard([&] {
        VR_CHECK(frame_min && weight_out && T > 0 && n_cuts >= 0 && (cuts || n_cuts == 0), VR_ERR_BAD_ARGUMENT, "null argument");
        int step = 0;
        for (int k = 0, at = 0; k <= n_cuts; ++k) {
            const int to = k < n_cuts ? cuts[k] : T;
            VR_CHECK(to >= at && to <= T && to > 0, VR_ERR_BAD_ARGUMENT, "cuts must ascend inside (0, T]");
            step = std::max(step, to - at);
            at = to;
        }
        const int RW = vr::kStreamPostDelay + step;
        std::vector<float> ring((size_t)RW, 0.f);
        vr::StreamPostState st{};
        int final_n = 0;
        auto declare = [&](int n) { for (; final_n < n; ++final_n) weight_out[final_n] = ring[(size_t)(final_n % RW)]; };
        for (int k = 0; k <= n_cuts; ++k) {
            const int to = k < n_cuts ? cuts[k] : T;
            vr::stream_post_advance(st, frame_min + st.h, to - st.h, ring.data(), RW);
            if (k < n_cuts) {
                declare(std::max(0, to - vr::kStreamPostDelay));
                if (final_after_out) final_after_out[k] = final_n;
            }
        }
        vr::stream_post_finish(st, ring.data(), RW);
        declare(T);
        if (final_after_out) final_after_out[n_cuts] = final_n;
    });
}

int vr_debug_record_taps(vr_handle h, int enable) {
    NEED(h);
    return guard([&] { h->m.record_taps = enable != 0; if (!enable) h->m.taps.clear(); });
}

int64_t vr_debug_get_tap(vr_handle h, const char* name, float* host, int64_t capacity_floats, int64_t* shape4) {
    if (!h || !name) { g_err = "null argument"; return VR_ERR_BAD_ARGUMENT; }
    int64_t n = 0;
    const int rc = guard([&] { n = h->m.get_tap(name, host, capacity_floats, shape4); });
    return rc == VR_OK ? n : rc;
}

}  // extern "C"
