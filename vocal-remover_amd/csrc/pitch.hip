// Pitch-shifted waves and training pairs (vr_pitch_*): the reference's augment.py without its external binary.
//
// The shift of one signal of L samples is librosa.effects.pitch_shift's:
//   D  = stft(y, n_fft, hop)                              stft_kernel, every signal of the item in one grid
//   D' = phase_vocoder(D, rate)                           augment_kernel<PitchVocoder> (augment.hip), fp64 phase
//   ys = istft(D', hop, length = round(L / rate))         istft_frame_kernel + istft_ola_kernel
//   z  = fix_length(resample(ys, ratio), L)               resample_kernel<ResampleFix> (audio.hip)
// and a training pair is y' = shift(y), v' = shift(X - y), X' = y' + v' (the sum formed by the resample kernel), then the STFTs of X'
// and y' at the handle's n_fft / hop.  This file is the host side: the lengths, the workspace and the order of the launches.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "model.h"

namespace vr {

void resample_table_create(double ratio, double** win, double** delta, int* nwin);
void launch_resample_fix(const float* x, long long n_in, int channels, double ratio, const double* win, const double* delta, int nwin, float* y,
                         float* sum, long long n_out, hipStream_t st);

// The four lengths of one shift, from the very expressions the launches use (vr_pitch_plan).
PitchPlan pitch_plan(long long L, int n_fft, int hop, double rate, double ratio) {
    VR_CHECK(n_fft > 0 && hop > 0, -2, "pitch: n_fft and hop must be positive");
    VR_CHECK(L >= n_fft, -2, "pitch: the wave has " + std::to_string(L) + " samples, fewer than n_fft = " + std::to_string(n_fft));
    VR_CHECK(rate > 0.0 && std::isfinite(rate) && ratio > 0.0 && std::isfinite(ratio), -2, "pitch: rate and ratio must be positive");
    VR_CHECK(L / hop < (1LL << 28) && (double)L / rate < 9.0e15 && (double)(1 + L / hop) / rate < (double)(1 << 30), -2, "pitch: wave too long");
    PitchPlan p;
    p.T = 1 + (int)(L / hop);
    p.T_stretch = (int)std::ceil((double)p.T / rate);                    // len(np.arange(0, T, rate))
    p.n_stretch = (long long)std::nearbyint((double)L / rate);           // int(round(L / rate)): half to even, like Python's round
    p.n_resampled = (long long)std::ceil((double)p.n_stretch * ratio);   // librosa.resample's length, before fix_length(L)
    VR_CHECK(p.n_stretch > 0, -2, "pitch: the stretched wave is empty");
    return p;
}

namespace {

struct DevBuf {                   // one allocation, freed on every way out
    char* p = nullptr;
    ~DevBuf() { hipFree(p); }
};

struct Carve {                    // 256-byte aligned pieces of it (or, base null, only their total)
    char* base;
    size_t off = 0;
    explicit Carve(char* b) : base(b) {}
    float* f(size_t n) {
        const size_t a = (off + 255) & ~size_t(255);
        off = a + n * sizeof(float);
        return base ? reinterpret_cast<float*>(base + a) : nullptr;
    }
};

struct ItemBufs { float *wave, *a, *b, *ys, *o0, *o1, *sx, *sy; };

// the buffers of one item: wave [S][L]; a = D [S][bins][T] complex64, then the frames [S][T'][n_fft]; b = D' [S][bins][T'] complex64;
// ys [S][n_stretch]; o0 / o1 [channels][L] = y' (the shifted wave) and X'; sx / sy = the two final spectrograms unless stored in place
ItemBufs carve_item(Carve& c, const PitchPlan& p, int S, int channels, long long L, int n_fft, bool pair, size_t final_floats) {
    const size_t bins = (size_t)n_fft / 2 + 1;
    ItemBufs b;
    b.wave = c.f((size_t)S * L);
    b.a = c.f(std::max((size_t)S * bins * p.T * 2, (size_t)S * p.T_stretch * n_fft));
    b.b = c.f((size_t)S * bins * p.T_stretch * 2);
    b.ys = c.f((size_t)S * p.n_stretch);
    b.o0 = c.f((size_t)channels * L);
    b.o1 = pair ? c.f((size_t)channels * L) : nullptr;
    b.sx = final_floats ? c.f(final_floats) : nullptr;
    b.sy = final_floats ? c.f(final_floats) : nullptr;
    return b;
}

}  // namespace

void Model::phase_vocoder_api(const float* spec, bool on_dev, int signals, int T, double rate, float* out, bool out_on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(signals > 0 && signals <= 65535 && T > 0, -2, "phase_vocoder: bad shape");
    VR_CHECK(rate > 0.0 && std::isfinite(rate) && (double)T / rate < (double)(1 << 30), -2, "phase_vocoder: rate must be positive");
    const int Tout = (int)std::ceil((double)T / rate);
    const size_t in_f = (size_t)signals * output_bin * T * 2, out_f = (size_t)signals * output_bin * Tout * 2;
    ensure_io((in_f + out_f) * sizeof(float) + 8192);
    io.reset();
    const float* sd = spec;
    if (!on_dev) {
        float* tmp = io.allocf(in_f);
        VR_HIP(hipMemcpyAsync(tmp, spec, in_f * sizeof(float), hipMemcpyHostToDevice, stream));
        sd = tmp;
    }
    float* od = out_on_dev ? out : io.allocf(out_f);
    launch_phase_vocoder(reinterpret_cast<const float2*>(sd), reinterpret_cast<float2*>(od), signals, output_bin, T, Tout, hop, rate, stream);
    if (!out_on_dev) VR_HIP(hipMemcpyAsync(out, od, out_f * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
}

void Model::istft_length_api(const float* spec, bool on_dev, int T, long long length, float* wave, bool wave_on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(T > 0 && length > 0, -2, "istft: empty spectrogram or length");
    const size_t spec_f = (size_t)2 * output_bin * T * 2, out_f = (size_t)2 * length, frames_f = (size_t)2 * T * n_fft;
    ensure_io((spec_f + out_f + frames_f) * sizeof(float) + 8192);
    io.reset();
    const float* sd = spec;
    if (!on_dev) {
        float* tmp = io.allocf(spec_f);
        VR_HIP(hipMemcpyAsync(tmp, spec, spec_f * sizeof(float), hipMemcpyHostToDevice, stream));
        sd = tmp;
    }
    float* frames = io.allocf(frames_f);
    float* wd = wave_on_dev ? wave : io.allocf(out_f);
    launch_istft_length(plan, reinterpret_cast<const float2*>(sd), hop, T, 2, frames, wd, length, stream);
    if (!wave_on_dev) VR_HIP(hipMemcpyAsync(wave, wd, out_f * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
}

void Model::pitch_run(int n, const float* const* waves, const float* const* inst, bool on_dev, int channels, const long long* L, int shift_n_fft,
                      int shift_hop, double rate, double ratio, long long max_bytes, float* const* out, float* const* X_out, float* const* y_out,
                      int layout, bool out_on_dev) {
    const bool pair = inst != nullptr;
    const std::string who = pair ? "pitch pair: " : "pitch shift: ";
    VR_CHECK(n > 0 && waves && L, -2, who + "no item");
    VR_CHECK(channels > 0 && channels <= 16384, -2, who + "bad channel count");
    VR_CHECK(!pair || channels == 2, -2, who + "a pair is two stereo waves");
    VR_CHECK(shift_n_fft >= 64 && (shift_n_fft & (shift_n_fft - 1)) == 0 && shift_n_fft <= 8192 && shift_hop > 0 && shift_hop <= shift_n_fft, -2,
             who + "the shift's n_fft must be a power of two in [64, 8192] and its hop in [1, n_fft]");
    VR_CHECK(layout == 0 || layout == 1, -2, who + "layout must be VR_PSEUDO_SPEC or VR_PSEUDO_ROWS");
    const bool rows = pair && layout == 1;
    VR_CHECK(!rows || istft_masked_available(plan, hop), -2,
             who + "the rows layout is a form of the frame-tiled STFT, which this handle does not have (hop_length == n_fft / 2 needed)");
    const int S = pair ? 4 : channels;
    DeviceGuard dev_guard(device);
    // everything is checked and sized before anything is allocated
    std::vector<PitchPlan> plans((size_t)n);
    size_t need = 0;
    for (int i = 0; i < n; ++i) {
        VR_CHECK(waves[i] && (!pair || inst[i]), -2, who + "null input " + std::to_string(i));
        VR_CHECK(pair ? (X_out && y_out && X_out[i] && y_out[i]) : (out && out[i]), -2, who + "null output " + std::to_string(i));
        plans[i] = pitch_plan(L[i], shift_n_fft, shift_hop, rate, ratio);
        VR_CHECK(!pair || L[i] / hop < (1LL << 28), -2, who + "wave too long");
        const size_t final_f = pair && !out_on_dev ? (size_t)2 * output_bin * (1 + L[i] / hop) * 2 : 0;
        Carve c(nullptr);
        carve_item(c, plans[i], S, channels, L[i], shift_n_fft, pair, final_f);
        need = std::max(need, c.off + 256);
    }
    size_t budget = 0;
    if (max_bytes > 0) budget = (size_t)max_bytes;
    else {
        size_t free_b = 0, total_b = 0;
        VR_HIP(hipMemGetInfo(&free_b, &total_b));
        budget = free_b - free_b / 10;
    }
    VR_CHECK(need <= budget, -4, who + "the largest item needs " + std::to_string(need) + " bytes of device workspace (" +
                                 std::to_string(need >> 20) + " MiB: its spectrogram at hop " + std::to_string(shift_hop) +
                                 ", the stretched one and the inverse transform's frames), the budget allows " + std::to_string(budget) +
                                 (max_bytes > 0 ? " (max_bytes)" : " (nine tenths of the free device memory)") + "; split the wave");
    const FFTPlan* sp = &plan;
    if (shift_n_fft != n_fft) {
        if (shift_plan.n_fft != shift_n_fft) {
            hipFree(shift_plan.twiddle); hipFree(shift_plan.window);
            shift_plan = FFTPlan{};                     // (fft_plan_create fills a plan only once both tables are on the device)
            fft_plan_create(shift_plan, shift_n_fft);
        }
        sp = &shift_plan;
    }
    const int sbins = shift_n_fft / 2 + 1;
    DevBuf buf, tw, td;
    VR_HIP(hipMalloc(&buf.p, need));
    int nwin = 0;
    {
        double *w = nullptr, *d = nullptr;
        resample_table_create(ratio, &w, &d, &nwin);
        tw.p = reinterpret_cast<char*>(w); td.p = reinterpret_cast<char*>(d);
    }
    const double* win = reinterpret_cast<const double*>(tw.p);
    const double* delta = reinterpret_cast<const double*>(td.p);
    const hipMemcpyKind in_kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = out_on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int i = 0; i < n; ++i) {
        const PitchPlan& p = plans[i];
        const long long Li = L[i];
        const int Tf = 1 + (int)(Li / hop);
        const size_t final_f = pair ? (size_t)2 * output_bin * Tf * 2 : 0;
        Carve c(buf.p);
        const ItemBufs b = carve_item(c, p, S, channels, Li, shift_n_fft, pair, pair && !out_on_dev ? final_f : 0);
        const size_t wave_bytes = (size_t)channels * Li * sizeof(float);
        if (pair) {                                     // rows 0, 1 = the instrumental, rows 2, 3 = mixture - instrumental
            VR_HIP(hipMemcpyAsync(b.wave, inst[i], wave_bytes, in_kind, stream));
            const float* mix = waves[i];
            if (!on_dev) {
                VR_HIP(hipMemcpyAsync(b.o1, waves[i], wave_bytes, hipMemcpyHostToDevice, stream));
                mix = b.o1;
            }
            launch_pitch_diff(mix, b.wave, b.wave + (size_t)2 * Li, 2 * Li, stream);
        } else {
            VR_HIP(hipMemcpyAsync(b.wave, waves[i], wave_bytes, in_kind, stream));
        }
        launch_stft_signals(*sp, b.wave, Li, shift_hop, p.T, S, reinterpret_cast<float2*>(b.a), stream);
        launch_phase_vocoder(reinterpret_cast<const float2*>(b.a), reinterpret_cast<float2*>(b.b), S, sbins, p.T, p.T_stretch, shift_hop, rate, stream);
        launch_istft_length(*sp, reinterpret_cast<const float2*>(b.b), shift_hop, p.T_stretch, S, b.a, b.ys, p.n_stretch, stream);
        launch_resample_fix(b.ys, p.n_stretch, channels, ratio, win, delta, nwin, b.o0, pair ? b.o1 : nullptr, Li, stream);
        if (!pair) {
            VR_HIP(hipMemcpyAsync(out[i], b.o0, wave_bytes, out_kind, stream));
            continue;
        }
        float* sx = out_on_dev ? X_out[i] : b.sx;
        float* sy = out_on_dev ? y_out[i] : b.sy;
        if (rows) {
            launch_stft_rows(plan, b.o1, Li, Tf, reinterpret_cast<float2*>(sx), stream);
            launch_stft_rows(plan, b.o0, Li, Tf, reinterpret_cast<float2*>(sy), stream);
        } else {
            launch_stft(plan, b.o1, Li, hop, Tf, reinterpret_cast<float2*>(sx), stream);
            launch_stft(plan, b.o0, Li, hop, Tf, reinterpret_cast<float2*>(sy), stream);
        }
        if (!out_on_dev) {
            VR_HIP(hipMemcpyAsync(X_out[i], sx, final_f * sizeof(float), hipMemcpyDeviceToHost, stream));
            VR_HIP(hipMemcpyAsync(y_out[i], sy, final_f * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
    }
    // one wait for the call: the items follow each other on the handle's stream, which orders every reuse of the workspace
    VR_HIP(hipStreamSynchronize(stream));
}

}  // namespace vr
