// Audio front end of inference.py / dataset preparation on the device:
//
//   vr_resample       the resampling step of librosa.load(path, sr=44100, res_type='kaiser_fast')
//                     (inference.py:136-138, lib/spec_utils.py:139-142).  librosa delegates to resampy 0.4
//                     (requirements.txt: resampy~=0.4.0, NOT vendored in the reference => parity unpinned): band-limited
//                     sinc interpolation with a Kaiser-windowed filter table -- 'kaiser_fast' = 16 zero crossings,
//                     2^9 table samples per crossing, roll-off 0.85, Kaiser beta 8.555504641634386 -- linear interpolation
//                     between table entries, left wing + right wing per output sample (resampy/interpn.py).
//   vr_resampler_*    the same resampler on blocks: a session with bounded state whose output, concatenated, is vr_resample's bit
//                     for bit; one launch serves any number of sessions.
//   vr_xcorr_argmax   argmax of np.correlate(a, b, 'full') in spec_utils.align_wave_head_and_tail
//                     (lib/spec_utils.py:107-108): one workgroup per lag.
// All are tiny next to the network; they exist so that the whole of inference.py / cache_or_load stays on the device
// path and needs neither librosa nor resampy.
#include <climits>
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.h"
#include "pcm.h"

namespace vr {

template <class A> __device__ __forceinline__ A resample_first(A a) { return a; }

// One session's share of a streamed launch (resample_kernel<true>, blockIdx.z selects the entry).  Every position is a global one: input
// sample g of the session lies at x[c * x_pitch + (g - g0)], output sample t0 + j goes to y[c * y_pitch + j].
struct ResampleSeg {
    const float* x;          // the window: [channels][x_pitch]
    long long x_pitch;
    long long g0;            // global index of the window's first sample
    long long n_in;          // samples received so far: the right-hand clamp.  Before the flush it is inactive for every sample launched
                             // (the host launches t only once input n(t) + K has arrived), at the flush it is the offline call's n_in
    long long t0;            // first output index of this launch
    long long count;         // output samples of this launch; a workgroup past it leaves at once
    long long t_core;        // outputs at or beyond it are librosa's zero tail (fix_length); LLONG_MAX before the flush
    float* y;
    long long y_pitch;
    const double* win;       // the session's filter table and its first differences
    const double* delta;
    double ratio;
    int nwin, precision;
};

// The PCM form's entry beside a ResampleSeg (resample_kernel<true, const ResamplePcm*>): the session's window is the float
// history x[0, blk_w) followed by the push's block as interleaved sample bytes, and the launch itself moves the decoded part of the carry on.
struct ResamplePcm {
    const uint8_t* bytes;    // the block: frames of `channels` samples (1: every session channel reads the one sample) in format `fmt`
    long long blk_w;         // window index of the block's first frame (= the float history held)
    float* carry;            // where window samples [carry_w, carry_w + carry_n) go, channel pitch x_pitch: the other window buffer
    long long carry_w, carry_n;
    int channels, fmt;
    int same;                // pass-through session: output sample t IS input sample t
};
// a channel's window of the PCM form, indexed like the float window
struct ResamplePcmWin {
    const float* x;
    const uint8_t* bytes;
    long long blk_w;
    int channels, fmt, ch;
    __device__ __forceinline__ float operator[](long long i) const { return i < blk_w ? x[i] : pcm_decode(bytes, fmt, channels, i - blk_w, ch); }
};

// One output sample: the sum over both filter wings (resampy.interpn._resample_loop), fp32 accumulator like the float32 output array.
// xc is the channel's window (a float pointer, or the PCM form's ResamplePcmWin), whose first sample has the global index g0; n_in is the
// right-hand clamp.
template <class WIN>
__device__ __forceinline__ float resample_sample(WIN xc, long long g0, long long n_in, long long t,
                                                 const double* __restrict__ win, const double* __restrict__ delta, int nwin, int precision,
                                                 double sample_ratio) {
    const double scale = sample_ratio < 1.0 ? sample_ratio : 1.0;
    const double time_increment = 1.0 / sample_ratio;
    const int index_step = (int)(scale * precision);
    const double time_register = (double)t * time_increment;
    const long long n = (long long)time_register;
    const long long nw = n - g0;                        // n inside the window
    double frac = scale * (time_register - (double)n);
    double index_frac = frac * precision;
    int offset = (int)index_frac;
    double eta = index_frac - offset;
    float acc = 0.f;
    long long i_max = (nwin - offset) / index_step;
    if (i_max > n + 1) i_max = n + 1;
    for (long long i = 0; i < i_max; ++i) {
        const int k = offset + (int)i * index_step;
        const double w = win[k] + eta * delta[k];
        acc = (float)((double)acc + w * (double)xc[nw - i]);
    }
    frac = scale - frac;
    index_frac = frac * precision;
    offset = (int)index_frac;
    eta = index_frac - offset;
    long long k_max = (nwin - offset) / index_step;
    if (k_max > n_in - n - 1) k_max = n_in - n - 1;
    for (long long k2 = 0; k2 < k_max; ++k2) {
        const int k = offset + (int)k2 * index_step;
        const double w = win[k] + eta * delta[k];
        acc = (float)((double)acc + w * (double)xc[nw + k2 + 1]);
    }
    return acc;
}

// y[c][t] = resample_sample of channel c.
// resample_kernel<false> is the offline kernel of vr_resample, argument for argument.  resample_kernel<true> takes a table of ResampleSeg
// in place of the first pointer (the other arguments are unused) and computes the same taps from global positions: output sample t
// depends on t alone, so a sample whose right wing lies inside the samples received is already the offline call's sample.
// PCM (at most one type, a trailing pack so that the two forms above keep their signatures and names): const ResamplePcm* (kStream only) = one
// entry per session beside the table.  Thread j < carry_n first stores window sample carry_w + j, decoded, into the other window buffer
// (the part of the carry that lies in the block; the float part is a device copy), then the output sample as above with the window read
// through ResamplePcmWin.  The grid covers max(count, carry_n), so the launch also happens for a push that returns no sample.
template <bool kStream, class... PCM>
__global__ void resample_kernel(std::conditional_t<kStream, const ResampleSeg*, const float*> __restrict__ x, long long n_in,
                                float* __restrict__ y, long long n_out, const double* __restrict__ win, const double* __restrict__ delta,
                                int nwin, int precision, double sample_ratio, PCM... pcm) {
    static_assert(sizeof...(PCM) == 0 || (sizeof...(PCM) == 1 && kStream), "one PCM table at most, for the streamed form");
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if constexpr (sizeof...(PCM) == 1) {
        const ResampleSeg& s = x[blockIdx.z];
        const ResamplePcm& q = resample_first(pcm...)[blockIdx.z];
        const ResamplePcmWin w{s.x + (long long)c * s.x_pitch, q.bytes, q.blk_w, q.channels, q.fmt, c < q.channels ? c : q.channels - 1};
        if (t < q.carry_n) q.carry[(long long)c * s.x_pitch + t] = w[q.carry_w + t];
        if (t >= s.count) return;
        float* yo = s.y + (long long)c * s.y_pitch + t;
        t += s.t0;
        if (t >= s.t_core) *yo = 0.f;
        else if (q.same) *yo = w[t - s.g0];
        else *yo = resample_sample(w, s.g0, s.n_in, t, s.win, s.delta, s.nwin, s.precision, s.ratio);
        return;
    }
    const float* xc;
    float* yo;
    long long g0 = 0;
    if constexpr (kStream) {
        const ResampleSeg& s = x[blockIdx.z];
        if (t >= s.count) return;
        yo = s.y + (long long)c * s.y_pitch + t;
        t += s.t0;
        if (t >= s.t_core) {
            *yo = 0.f;
            return;
        }
        xc = s.x + (long long)c * s.x_pitch;
        g0 = s.g0;
        n_in = s.n_in;
        win = s.win;
        delta = s.delta;
        nwin = s.nwin;
        precision = s.precision;
        sample_ratio = s.ratio;
    } else {
        if (t >= n_out) return;
        xc = x + (long long)c * n_in;
        yo = y + (long long)c * n_out + t;
    }
    *yo = resample_sample(xc, g0, n_in, t, win, delta, nwin, precision, sample_ratio);
}

// The pitch form (librosa.effects.pitch_shift's resample + fix_length): channel c of x [rows][n_in] -> y [c][n_out],
// samples [0, n_core) computed (n_core = min(int(n_in * ratio), n_out)), zeros behind them.  `sum` (the pair entry): x holds 2 * gridDim.y
// rows, the instrumental's then the vocals'; sum[c][t] = y[c][t] + the vocals' sample, one float32 addition -- the rebuilt mixture
// X' = y' + v' costs no pass of its own.
struct ResampleFix {
    const float* x;
    long long n_in, n_core, n_out;
    float* y;
    float* sum;               // or null
    const double* win;
    const double* delta;
    int nwin, precision;
    double ratio;
};

template <class FORM>
__global__ void resample_kernel(FORM f) {
    static_assert(std::is_same<FORM, ResampleFix>::value, "resample_kernel: unknown form");
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (t >= f.n_out) return;
    const long long o = (long long)c * f.n_out + t;
    float a = 0.f, b = 0.f;
    if (t < f.n_core) {
        a = resample_sample(f.x + (long long)c * f.n_in, 0, f.n_in, t, f.win, f.delta, f.nwin, f.precision, f.ratio);
        if (f.sum) b = resample_sample(f.x + (long long)(c + gridDim.y) * f.n_in, 0, f.n_in, t, f.win, f.delta, f.nwin, f.precision, f.ratio);
    }
    f.y[o] = a;
    if (f.sum) f.sum[o] = a + b;
}

// resampy.filters.sinc_window(num_zeros, precision, kaiser(beta), rolloff): the right half of the windowed sinc
static void kaiser_sinc_table(int num_zeros, int precision_bits, double rolloff, double beta, std::vector<double>& win) {
    const int num_bits = 1 << precision_bits;
    const int n = num_bits * num_zeros;
    win.resize((size_t)n + 1);
    const double PI = 3.14159265358979323846;
    const double i0b = std::cyl_bessel_i(0.0, beta);
    for (int k = 0; k <= n; ++k) {
        const double xs = rolloff * ((double)num_zeros * k / n);                    // linspace(0, num_zeros, n+1) * rolloff
        const double sinc = xs == 0.0 ? 1.0 : std::sin(PI * xs) / (PI * xs);
        const double r = (double)k / n;                                             // kaiser(2n+1, beta)[n + k]
        const double taper = std::cyl_bessel_i(0.0, beta * std::sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / i0b;
        win[k] = taper * rolloff * sinc;
    }
}

// the 'kaiser_fast' table as the kernels read it for one ratio: scaled by the ratio when it decimates, and its first differences
static void kaiser_fast_table(double ratio, std::vector<double>& win, std::vector<double>& delta) {
    kaiser_sinc_table(16, 9, 0.85, 8.555504641634386, win);
    if (ratio < 1.0) for (double& v : win) v *= ratio;
    delta.resize(win.size());
    for (size_t i = 0; i + 1 < win.size(); ++i) delta[i] = win[i + 1] - win[i];
    delta.back() = 0.0;
}

// vr_resample_ratio: the resampler for a ratio that is no quotient of two integer rates (librosa.effects.pitch_shift resamples by
// sr / (sr / rate)); vr_resample is this with ratio = (double)sr_out / sr_in
void resample_ratio_api(int device, const float* x, int channels, long long n_in, double ratio, float* y, long long n_out) {
    VR_CHECK(channels > 0 && n_in > 0 && ratio > 0.0 && n_out > 0, -2, "resample: bad argument");
    VR_CHECK((int)((ratio < 1.0 ? ratio : 1.0) * (1 << 9)) >= 1, -2, "resample: the ratio is below the filter table's resolution (1 / 512)");
    DeviceGuard dev_guard(device);
    VR_CHECK(n_out <= (long long)std::ceil((double)n_in * ratio) + 1, -2, "resample: n_out larger than ceil(n_in * ratio)");
    std::vector<double> win, delta;
    kaiser_fast_table(ratio, win, delta);
    float *dx = nullptr, *dy = nullptr;
    double *dw = nullptr, *dd = nullptr;
    struct Free { void* p[4]; ~Free() { for (void* q : p) hipFree(q); } } fr{{nullptr, nullptr, nullptr, nullptr}};
    VR_HIP(hipMalloc(&dx, (size_t)channels * n_in * sizeof(float))); fr.p[0] = dx;
    VR_HIP(hipMalloc(&dy, (size_t)channels * n_out * sizeof(float))); fr.p[1] = dy;
    VR_HIP(hipMalloc(&dw, win.size() * sizeof(double))); fr.p[2] = dw;
    VR_HIP(hipMalloc(&dd, win.size() * sizeof(double))); fr.p[3] = dd;
    VR_HIP(hipMemcpy(dx, x, (size_t)channels * n_in * sizeof(float), hipMemcpyHostToDevice));
    VR_HIP(hipMemcpy(dw, win.data(), win.size() * sizeof(double), hipMemcpyHostToDevice));
    VR_HIP(hipMemcpy(dd, delta.data(), win.size() * sizeof(double), hipMemcpyHostToDevice));
    // resampy produces int(n_in * ratio) samples; librosa's fix_length pads / trims to ceil(n_in * ratio) with zeros
    const long long n_core = (long long)((double)n_in * ratio);
    VR_HIP(hipMemset(dy, 0, (size_t)channels * n_out * sizeof(float)));
    const long long n_run = n_core < n_out ? n_core : n_out;
    if (n_run > 0) {
        float* ytmp = dy;
        // rows of dy are n_out long; the kernel writes the first n_run samples of each
        hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)((n_run + 255) / 256), channels), dim3(256), 0, 0, dx, n_in, ytmp, n_out,
                           dw, dd, (int)win.size(), 1 << 9, ratio);
        VR_HIP(hipGetLastError());
    }
    VR_HIP(hipDeviceSynchronize());
    // samples [n_run, n_out) of every row must stay zero: the kernel guards t < n_out only, so clear the tail again
    if (n_run < n_out)
        for (int c = 0; c < channels; ++c)
            VR_HIP(hipMemset(dy + (size_t)c * n_out + n_run, 0, (size_t)(n_out - n_run) * sizeof(float)));
    VR_HIP(hipMemcpy(y, dy, (size_t)channels * n_out * sizeof(float), hipMemcpyDeviceToHost));
}

void resample_api(int device, const float* x, int channels, long long n_in, int sr_in, int sr_out, float* y, long long n_out) {
    VR_CHECK(sr_in > 0 && sr_out > 0, -2, "resample: bad argument");
    resample_ratio_api(device, x, channels, n_in, (double)sr_out / (double)sr_in, y, n_out);
}

// ---- the pitch form: the filter table of one call on the device, and the launch (csrc/pitch.hip) ------------------------------------
void resample_table_create(double ratio, double** win, double** delta, int* nwin) {
    VR_CHECK(ratio > 0.0 && (int)((ratio < 1.0 ? ratio : 1.0) * (1 << 9)) >= 1, -2,
             "pitch: the resampling ratio is below the filter table's resolution (1 / 512)");
    std::vector<double> w, d;
    kaiser_fast_table(ratio, w, d);
    *win = *delta = nullptr;
    VR_HIP(hipMalloc(win, w.size() * sizeof(double)));
    VR_HIP(hipMalloc(delta, w.size() * sizeof(double)));
    VR_HIP(hipMemcpy(*win, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    VR_HIP(hipMemcpy(*delta, d.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    *nwin = (int)w.size();
}

// x [rows][n_in] -> y [channels][n_out] = fix_length(resample(x, ratio), n_out); sum (or null): x has 2 * channels rows, sum = y + the
// resampled rows [channels, 2 channels)
void launch_resample_fix(const float* x, long long n_in, int channels, double ratio, const double* win, const double* delta, int nwin, float* y,
                         float* sum, long long n_out, hipStream_t st) {
    long long n_core = (long long)((double)n_in * ratio);
    if (n_core > n_out) n_core = n_out;
    prof_note(0.0, 4.0 * ((sum ? 2.0 : 1.0) * channels * (double)n_in + (sum ? 2.0 : 1.0) * channels * (double)n_out));
    VR_LAUNCH(resample_kernel<ResampleFix>, dim3((unsigned)((n_out + 255) / 256), (unsigned)channels), dim3(256), 0, st,
              ResampleFix{x, n_in, n_core, n_out, y, sum, win, delta, nwin, 1 << 9, ratio});
    VR_HIP(hipGetLastError());
}

// ---- the streamed resampler (vr_resampler_*) -------------------------------------------------------------------------------------
// The schedule, from the very expressions of resample_api and the kernel: ratio = (double)sr_out / sr_in, n(t) = (long long)((double)t *
// (1.0 / ratio)), K = nwin / index_step (no wing reaches further: a wing has (nwin - offset) / index_step <= K taps).  Output sample t
// reads the inputs n(t) - K + 1 .. n(t) + K at most, so it is final once input n(t) + K has arrived: from then on the right-hand clamp
// n_in - n - 1 is inactive whatever n_in turns out to be.  At the flush n_in is known: the rest is computed with the clamp active, up to
// resampy's int(n_in * ratio), and zeros follow up to librosa's ceil(n_in * ratio).
struct ResampleGeom {
    double ratio, inc;
    int index_step, K;
};

static ResampleGeom resample_geom(int sr_in, int sr_out) {
    VR_CHECK(sr_in > 0 && sr_out > 0, -2, "resampler: the sample rates must be positive");
    ResampleGeom g;
    g.ratio = (double)sr_out / (double)sr_in;
    g.inc = 1.0 / g.ratio;
    const double scale = g.ratio < 1.0 ? g.ratio : 1.0;
    g.index_step = (int)(scale * (1 << 9));
    VR_CHECK(g.index_step >= 1, -2, "resampler: sr_out / sr_in is below the filter table's resolution (1 / 512)");
    g.K = ((16 << 9) + 1) / g.index_step;
    return g;
}

static long long resample_ready(const ResampleGeom& g, long long samples_in, bool flushed) {
    VR_CHECK(samples_in >= 0, -2, "resampler: negative sample count");
    if (flushed) {
        VR_CHECK(samples_in > 0, -2, "resampler: flush with no sample received");
        return (long long)std::ceil((double)samples_in * g.ratio);
    }
    const long long m = samples_in - g.K - 1;                 // the last n(t) whose right wing has arrived whole
    if (m < 0) return 0;
    long long t = (long long)((double)(m + 1) * g.ratio);      // an estimate of the first t with n(t) > m, then the exact expression
    while ((long long)((double)t * g.inc) <= m) ++t;
    while (t > 0 && (long long)((double)(t - 1) * g.inc) > m) --t;
    return t;
}

long long resampler_plan(int sr_in, int sr_out, long long samples_in, bool flushed) {
    return resample_ready(resample_geom(sr_in, sr_out), samples_in, flushed);
}

// One session: its own stream, its filter table, two window buffers [channels][pitch] used in turn (the carried samples are copied
// from the front of one to the front of the other, so no copy overlaps itself), an output staging buffer for host destinations and a
// launch table.  The window buffers grow to history + the largest push seen; nothing else is allocated after the first pushes.
struct Resampler {
    int device, channels, sr_in, sr_out;
    ResampleGeom g;
    hipStream_t st = nullptr;
    double *d_win = nullptr, *d_delta = nullptr;
    int nwin = 0;
    float* buf[2] = {nullptr, nullptr};
    long long pitch = 0, hist = 0, g0 = 0;       // samples per row; samples held at the front of buf[cur]; global index of the first
    int cur = 0;
    long long n_recv = 0, n_emit = 0;            // the two counters: input samples received, output samples returned
    bool flushed = false, broken = false;
    float* d_out = nullptr;
    long long out_cap = 0;
    ResampleSeg *d_tab = nullptr, *h_tab = nullptr;
    int tab_cap = 0;
    uint8_t* d_pcm = nullptr;                    // (PCM pushes from the host) the block's bytes, staged as bytes
    size_t pcm_cap = 0;
    ResamplePcm *d_ptab = nullptr, *h_ptab = nullptr;
    int ptab_cap = 0;
    long long history_cap() const { return 2LL * g.K + 2; }
    ~Resampler() {
        hipFree(d_win); hipFree(d_delta); hipFree(buf[0]); hipFree(buf[1]); hipFree(d_out); hipFree(d_tab); hipFree(d_pcm); hipFree(d_ptab);
        if (h_tab) hipHostFree(h_tab);
        if (h_ptab) hipHostFree(h_ptab);
        if (st) hipStreamDestroy(st);
    }
};

Resampler* resampler_open(int device, int channels, int sr_in, int sr_out) {
    DeviceGuard dev_guard(device);
    Resampler* r = new Resampler();
    try {
        r->device = device; r->channels = channels; r->sr_in = sr_in; r->sr_out = sr_out;
        r->g = resample_geom(sr_in, sr_out);
        VR_HIP(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
        std::vector<double> win, delta;
        kaiser_fast_table(r->g.ratio, win, delta);                                    // as resample_api builds it
        r->nwin = (int)win.size();
        VR_HIP(hipMalloc(&r->d_win, win.size() * sizeof(double)));
        VR_HIP(hipMalloc(&r->d_delta, win.size() * sizeof(double)));
        VR_HIP(hipMemcpy(r->d_win, win.data(), win.size() * sizeof(double), hipMemcpyHostToDevice));
        VR_HIP(hipMemcpy(r->d_delta, delta.data(), win.size() * sizeof(double), hipMemcpyHostToDevice));
        r->pitch = r->history_cap();
        for (float*& b : r->buf) VR_HIP(hipMalloc(&b, (size_t)channels * r->pitch * sizeof(float)));
    } catch (...) {
        delete r;
        throw;
    }
    return r;
}

void resampler_close(Resampler* r) {
    DeviceGuard dev_guard(r->device);
    delete r;
}

void resampler_info(const Resampler* r, long long* lookahead, long long* state_bytes) {
    if (lookahead) *lookahead = r->g.K + 1;
    if (state_bytes)
        *state_bytes = (long long)r->channels * r->history_cap() * (long long)sizeof(float) + 2LL * r->nwin * (long long)sizeof(double) +
                       2LL * (long long)sizeof(long long);
}

static void copy_rows(void* dst, long long dpitch, const void* src, long long spitch, long long width, int rows, hipMemcpyKind kind,
                      hipStream_t st) {
    if (width > 0)
        VR_HIP(hipMemcpy2DAsync(dst, (size_t)dpitch * sizeof(float), src, (size_t)spitch * sizeof(float), (size_t)width * sizeof(float),
                                (size_t)rows, kind, st));
}

// Session k receives n[k] >= 0 samples and, where flush[k], its input ends.  Everything is checked first; then the copies of all sessions,
// ONE launch with one table entry per session, the copies out and the carry run on session 0's stream, and the call waits for it (every
// session's memory is idle between calls, so no other stream has to be waited for).
// pcm_fmt given (vr_resampler_push*_pcm; x is then unused): session k's block is bytes[k], n[k] interleaved frames of pcm_channels[k] samples
// in format pcm_fmt[k].  The window keeps only the float history: host bytes are staged as bytes in the session's own buffer, the PCM form of
// the kernel reads history and block, returns a pass-through session's samples too, and stores the decoded part of the carry itself -- so
// the launch also happens for a push that returns nothing.  What is left behind is the float state a float push leaves.
void resampler_push_many(int N, Resampler* const* r, const float* const* x, bool x_on_dev, const long long* n, const int* flush,
                         float* const* y, bool y_on_dev, const long long* capacity, long long* n_out, bool many, const void* const* bytes,
                         const int* pcm_channels, const int* pcm_fmt) {
    VR_CHECK(N <= 65535, -2, "resampler: at most 65535 sessions in one call (one grid plane each)");
    const bool pcm = pcm_fmt != nullptr;
    VR_CHECK(!pcm || pcm_channels, -2, "resampler: null table");
    std::vector<long long> need((size_t)N, 0), total((size_t)N, 0);
    for (int k = 0; k < N; ++k) {
        const std::string who = many ? "resampler " + std::to_string(k) + ": " : std::string("resampler: ");
        VR_CHECK(r[k], -2, who + "null session (closed?)");
        for (int j = 0; j < k; ++j) VR_CHECK(r[j] != r[k], -2, who + "the same session as resampler " + std::to_string(j));
        VR_CHECK(r[k]->device == r[0]->device, -2, who + "on another device than resampler 0: the sessions of one call share a device");
        VR_CHECK(r[k]->channels == r[0]->channels, -2, who + "another channel count than resampler 0");
        const bool fl = flush && flush[k];
        VR_CHECK(!r[k]->flushed, -2, who + (fl && n[k] == 0 ? "already flushed" : "push after flush"));
        VR_CHECK(!r[k]->broken, -2, who + "an earlier call failed half way: close the session");
        VR_CHECK(n[k] >= 0, -2, who + "negative sample count");
        if (pcm) {
            VR_CHECK(pcm_fmt_ok(pcm_fmt[k]), -2, who + "unknown sample format " + std::to_string(pcm_fmt[k]) + " (VR_PCM_S16 / S24 / S32 / F32)");
            VR_CHECK(pcm_channels[k] == 1 || pcm_channels[k] == r[k]->channels, -2,
                     who + "frames of " + std::to_string(pcm_channels[k]) + " channels: a block holds the session's " + std::to_string(r[k]->channels) +
                         " or 1 (every session channel then reads the one sample)");
            VR_CHECK(n[k] == 0 || (bytes && bytes[k]), -2, who + "null input");
            if (x_on_dev && n[k] > 0 && pcm_fmt[k] != VR_PCM_S24)
                VR_CHECK(reinterpret_cast<uintptr_t>(bytes[k]) % (uintptr_t)pcm_sample_bytes(pcm_fmt[k]) == 0, -2,
                         who + "the sample buffer is not aligned to its " + std::to_string(pcm_sample_bytes(pcm_fmt[k])) +
                             "-byte samples (only VR_PCM_S24 may start at any byte)");
        } else
            VR_CHECK(n[k] == 0 || (x && x[k]), -2, who + "null input");
        total[k] = r[k]->n_recv + n[k];
        VR_CHECK(!fl || total[k] > 0, -2, who + "flush with no sample received");
        need[k] = resample_ready(r[k]->g, total[k], fl) - r[k]->n_emit;
        const long long cap = capacity ? capacity[k] : 0;
        VR_CHECK(cap >= need[k], -2, who + "capacity " + std::to_string(cap) + " but the call returns " + std::to_string(need[k]) + " samples");
        VR_CHECK(need[k] == 0 || (y && y[k]), -2, who + "null output");
    }
    Resampler* lead = r[0];
    const int C = lead->channels;
    DeviceGuard dev_guard(lead->device);
    hipStream_t st = lead->st;
    for (int k = 0; k < N; ++k) r[k]->broken = true;
    if (lead->tab_cap < N) {
        hipFree(lead->d_tab);
        if (lead->h_tab) hipHostFree(lead->h_tab);
        lead->d_tab = nullptr; lead->h_tab = nullptr; lead->tab_cap = 0;
        VR_HIP(hipMalloc(&lead->d_tab, (size_t)N * sizeof(ResampleSeg)));
        VR_HIP(hipHostMalloc(&lead->h_tab, (size_t)N * sizeof(ResampleSeg)));
        lead->tab_cap = N;
    }
    if (pcm && lead->ptab_cap < N) {
        hipFree(lead->d_ptab);
        if (lead->h_ptab) hipHostFree(lead->h_ptab);
        lead->d_ptab = nullptr; lead->h_ptab = nullptr; lead->ptab_cap = 0;
        VR_HIP(hipMalloc(&lead->d_ptab, (size_t)N * sizeof(ResamplePcm)));
        VR_HIP(hipHostMalloc(&lead->h_ptab, (size_t)N * sizeof(ResamplePcm)));
        lead->ptab_cap = N;
    }
    const hipMemcpyKind in_kind = x_on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = y_on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    long long max_count = 0;
    std::vector<long long> keep_at((size_t)N, 0);       // (PCM) the first global sample the session carries on
    for (int k = 0; k < N; ++k) {
        Resampler& s = *r[k];
        const bool fl = flush && flush[k];
        const bool same = s.sr_in == s.sr_out;               // pass-through: the schedule is the filter's, the samples are the input's
        if (pcm) {
            ResamplePcm& q = lead->h_ptab[k];
            q = ResamplePcm{};
            q.bytes = n[k] ? static_cast<const uint8_t*>(bytes[k]) : nullptr;
            if (!x_on_dev && n[k] > 0) {                    // staged as bytes; rounded so that pcm_load24's aligned word reads stay inside
                const size_t nb = (size_t)n[k] * pcm_channels[k] * pcm_sample_bytes(pcm_fmt[k]);
                if (s.pcm_cap < nb) {
                    hipFree(s.d_pcm); s.d_pcm = nullptr; s.pcm_cap = 0;
                    VR_HIP(hipMalloc(&s.d_pcm, ((nb + 3) & ~size_t(3)) + 4));
                    s.pcm_cap = nb;
                }
                VR_HIP(hipMemcpyAsync(s.d_pcm, bytes[k], nb, hipMemcpyHostToDevice, st));
                q.bytes = s.d_pcm;
            }
            q.blk_w = s.hist; q.channels = pcm_channels[k]; q.fmt = pcm_fmt[k]; q.same = same ? 1 : 0;
            ResampleSeg& e = lead->h_tab[k];
            e.x = s.buf[s.cur]; e.x_pitch = s.pitch; e.g0 = s.g0; e.n_in = total[k];
            e.t0 = s.n_emit; e.count = need[k];
            e.t_core = fl ? (long long)((double)total[k] * s.g.ratio) : LLONG_MAX;
            VR_CHECK(s.n_emit <= e.t_core, -3, "resampler: the schedule ran past int(n_in * ratio)");
            e.win = s.d_win; e.delta = s.d_delta; e.ratio = s.g.ratio; e.nwin = s.nwin; e.precision = 1 << 9;
            if (y_on_dev) { e.y = y[k]; e.y_pitch = capacity ? capacity[k] : 0; }
            else {
                if (s.out_cap < need[k]) {
                    hipFree(s.d_out); s.d_out = nullptr; s.out_cap = 0;
                    VR_HIP(hipMalloc(&s.d_out, (size_t)C * need[k] * sizeof(float)));
                    s.out_cap = need[k];
                }
                e.y = s.d_out; e.y_pitch = need[k];
            }
            VR_CHECK(e.count == 0 || s.g0 <= std::max(0LL, (long long)((double)e.t0 * s.g.inc) - s.g.K + 1), -3, "resampler: window lost its history");
            if (!fl && n[k] > 0) {
                // the carry (the rule below): its float part [keep, n_recv) is a device copy, the launch stores the decoded rest [d0, total)
                long long keep = std::max(s.g0, std::max(0LL, (long long)((double)(s.n_emit + need[k]) * s.g.inc) - s.g.K));
                keep = std::min(keep, total[k]);
                VR_CHECK(total[k] - keep <= s.pitch, -3, "resampler: the carry outgrew the window");
                keep_at[k] = keep;
                const long long d0 = std::max(keep, s.n_recv);
                q.carry = s.buf[1 - s.cur] + (d0 - keep); q.carry_w = d0 - s.g0; q.carry_n = total[k] - d0;
            }
            max_count = std::max(max_count, std::max(e.count, q.carry_n));
            continue;
        }
        if (s.hist + n[k] > s.pitch) {                      // a larger push than any before: both windows grow, the history moves over
            const long long pitch = s.history_cap() + n[k];
            struct Pair { float* p[2]; ~Pair() { hipFree(p[0]); hipFree(p[1]); } } nb{{nullptr, nullptr}};      // freed unless taken over
            for (float*& b : nb.p) VR_HIP(hipMalloc(&b, (size_t)C * pitch * sizeof(float)));
            copy_rows(nb.p[0], pitch, s.buf[s.cur], s.pitch, s.hist, C, hipMemcpyDeviceToDevice, st);
            VR_HIP(hipStreamSynchronize(st));
            std::swap(s.buf[0], nb.p[0]);                    // the old pair goes with the guard
            std::swap(s.buf[1], nb.p[1]);
            s.cur = 0; s.pitch = pitch;
        }
        copy_rows(s.buf[s.cur] + s.hist, s.pitch, n[k] ? x[k] : nullptr, n[k], n[k], C, in_kind, st);
        ResampleSeg& e = lead->h_tab[k];
        e.x = s.buf[s.cur]; e.x_pitch = s.pitch; e.g0 = s.g0; e.n_in = total[k];
        e.t0 = s.n_emit; e.count = same ? 0 : need[k];
        e.t_core = fl ? (long long)((double)total[k] * s.g.ratio) : LLONG_MAX;
        VR_CHECK(s.n_emit <= e.t_core, -3, "resampler: the schedule ran past int(n_in * ratio)");
        e.win = s.d_win; e.delta = s.d_delta; e.ratio = s.g.ratio; e.nwin = s.nwin; e.precision = 1 << 9;
        if (y_on_dev) { e.y = y[k]; e.y_pitch = capacity ? capacity[k] : 0; }
        else if (!same) {
            if (s.out_cap < need[k]) {
                hipFree(s.d_out); s.d_out = nullptr; s.out_cap = 0;
                VR_HIP(hipMalloc(&s.d_out, (size_t)C * need[k] * sizeof(float)));
                s.out_cap = need[k];
            }
            e.y = s.d_out; e.y_pitch = need[k];
        } else { e.y = nullptr; e.y_pitch = 0; }              // pass-through to the host: copied from the window, no staging
        // the first sample of the launch reads from n(t0) - K + 1 on: the carry rule below keeps it inside the window
        VR_CHECK(e.count == 0 || s.g0 <= std::max(0LL, (long long)((double)e.t0 * s.g.inc) - s.g.K + 1), -3, "resampler: window lost its history");
        max_count = std::max(max_count, e.count);
    }
    if (max_count > 0 && pcm) {
        VR_HIP(hipMemcpyAsync(lead->d_tab, lead->h_tab, (size_t)N * sizeof(ResampleSeg), hipMemcpyHostToDevice, st));
        VR_HIP(hipMemcpyAsync(lead->d_ptab, lead->h_ptab, (size_t)N * sizeof(ResamplePcm), hipMemcpyHostToDevice, st));
        float* const unused_out = nullptr;
        const double* const unused_tab = nullptr;
        const ResamplePcm* ptab = lead->d_ptab;
        VR_LAUNCH((resample_kernel<true, const ResamplePcm*>), dim3((unsigned)((max_count + 255) / 256), C, N), dim3(256), 0, st, lead->d_tab, 0LL,
                  unused_out, 0LL, unused_tab, unused_tab, 0, 0, 0.0, ptab);
        VR_HIP(hipGetLastError());
    } else if (max_count > 0) {
        VR_HIP(hipMemcpyAsync(lead->d_tab, lead->h_tab, (size_t)N * sizeof(ResampleSeg), hipMemcpyHostToDevice, st));
        float* const unused_out = nullptr;
        const double* const unused_tab = nullptr;
        VR_LAUNCH(resample_kernel<true>, dim3((unsigned)((max_count + 255) / 256), C, N), dim3(256), 0, st, lead->d_tab, 0LL, unused_out, 0LL,
                  unused_tab, unused_tab, 0, 0, 0.0);
        VR_HIP(hipGetLastError());
    }
    for (int k = 0; k < N; ++k) {
        Resampler& s = *r[k];
        const ResampleSeg& e = lead->h_tab[k];
        const long long cap = capacity ? capacity[k] : 0;
        if (pcm) {
            if (!y_on_dev) copy_rows(y ? y[k] : nullptr, cap, s.d_out, e.y_pitch, need[k], C, hipMemcpyDeviceToHost, st);
            if (!(flush && flush[k]) && n[k] > 0) {
                const long long keep = keep_at[k];
                copy_rows(s.buf[1 - s.cur], s.pitch, s.buf[s.cur] + (keep - s.g0), s.pitch, std::min(total[k], s.n_recv) - keep, C,
                          hipMemcpyDeviceToDevice, st);
                s.cur = 1 - s.cur; s.g0 = keep; s.hist = total[k] - keep;
            }
            continue;
        }
        if (s.sr_in == s.sr_out) copy_rows(y ? y[k] : nullptr, cap, s.buf[s.cur] + (s.n_emit - s.g0), s.pitch, need[k], C, out_kind, st);
        else if (!y_on_dev) copy_rows(y ? y[k] : nullptr, cap, s.d_out, e.y_pitch, need[k], C, hipMemcpyDeviceToHost, st);
        const bool fl = flush && flush[k];
        const long long emit = s.n_emit + need[k];
        if (!fl && n[k] > 0) {
            // the next sample to come, t = emit, reads from n(t) - K + 1 on; n(t) + K >= total (it is not final), so at most 2K are kept
            long long keep = std::max(s.g0, std::max(0LL, (long long)((double)emit * s.g.inc) - s.g.K));
            keep = std::min(keep, total[k]);
            copy_rows(s.buf[1 - s.cur], s.pitch, s.buf[s.cur] + (keep - s.g0), s.pitch, total[k] - keep, C, hipMemcpyDeviceToDevice, st);
            s.cur = 1 - s.cur; s.g0 = keep; s.hist = total[k] - keep;
        }
    }
    VR_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < N; ++k) {
        Resampler& s = *r[k];
        s.n_recv = total[k]; s.n_emit += need[k];
        if (flush && flush[k]) s.flushed = true;
        s.broken = false;
        if (n_out) n_out[k] = need[k];
    }
}

// full[k] = sum_n a[n + k - (nb - 1)] * b[n],  k = 0 .. na + nb - 2   (np.correlate(a, b, 'full'), real input)
__global__ __launch_bounds__(256) void xcorr_full_kernel(const float* __restrict__ a, long long na, const float* __restrict__ b,
                                                         long long nb, float* __restrict__ full) {
    const long long k = blockIdx.x;
    const long long shift = k - (nb - 1);
    long long lo = shift < 0 ? -shift : 0;                 // n with 0 <= n + shift < na
    long long hi = nb < na - shift ? nb : na - shift;
    float s = 0.f;
    for (long long n = lo + threadIdx.x; n < hi; n += 256) s = fmaf(a[n + shift], b[n], s);
    __shared__ float red[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) full[k] = red[0] + red[1] + red[2] + red[3];
}

void xcorr_argmax_api(int device, const float* a, long long na, const float* b, long long nb, long long* argmax_out) {
    VR_CHECK(na > 0 && nb > 0 && na + nb - 1 < 0x7FFFFFFFLL, -2, "xcorr: bad lengths");
    DeviceGuard dev_guard(device);
    const long long nf = na + nb - 1;
    float *da = nullptr, *db = nullptr, *df = nullptr;
    struct Free { void* p[3]; ~Free() { for (void* q : p) hipFree(q); } } fr{{nullptr, nullptr, nullptr}};
    VR_HIP(hipMalloc(&da, (size_t)na * sizeof(float))); fr.p[0] = da;
    VR_HIP(hipMalloc(&db, (size_t)nb * sizeof(float))); fr.p[1] = db;
    VR_HIP(hipMalloc(&df, (size_t)nf * sizeof(float))); fr.p[2] = df;
    VR_HIP(hipMemcpy(da, a, (size_t)na * sizeof(float), hipMemcpyHostToDevice));
    VR_HIP(hipMemcpy(db, b, (size_t)nb * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(xcorr_full_kernel, dim3((unsigned)nf), dim3(256), 0, 0, da, na, db, nb, df);
    VR_HIP(hipGetLastError());
    std::vector<float> full((size_t)nf);
    VR_HIP(hipMemcpy(full.data(), df, (size_t)nf * sizeof(float), hipMemcpyDeviceToHost));
    long long best = 0;
    for (long long k = 1; k < nf; ++k) if (full[(size_t)k] > full[(size_t)best]) best = k;       // np.argmax: first maximum
    *argmax_out = best;
}

}  // namespace vr
