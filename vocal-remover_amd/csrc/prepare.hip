// Plain training pairs on the device (vr_align_pair_many, vr_pair_rows_many): what the reference's
// spec_utils.cache_or_load does to a decoded (mixture, instrumental) pair -- trim each wave, cross-correlate the two heads, cut both to
// the common window, STFT both, take the pair's peak -- many pairs per call, in two steps with the window back on the host between them.
//
//   step 1, vr_align_pair_many (no handle; the call's table of 2 n waves, a grid dimension picks the wave or the pair):
//     PrepRms     rms of every librosa.effects.trim frame (2048 samples, hop 512, centre zero padding), squares summed in double
//     PrepTrim    ref = the largest rms, first / last frame within 60 dB of it -> start, end; the head's sum in double -> its mean
//     PrepHeads   head[j] = (w[0][start + j] + w[1][start + j]) - mean, the first min(4 sr, end - start) trimmed samples
//     XcorrTile   np.correlate(a, b, 'full') of the pair's two heads (one launch per pair: the only stage that is not a table launch)
//     LagPart, LagPick   the first maximum of it, in two launches -> lag = argmax - (na - 1)
//   One copy of n windows back, one wait.  The host finishes each window with pair_window_plan (kernels.h).
//   step 2, vr_pair_rows_many (a handle: its FFT plan and stream): the window of each wave copied into the workspace (the frame-tiled
//     STFT reads channels L apart: a copy, not a pitch argument), stft_tile_kernel<SpecRows> on both, launch_song_peak on the rows.
//
// No new kernel name: the six device forms are instantiations of a template that shares the name of the kernel whose arithmetic the lag
// search restates, xcorr_full_kernel (audio.hip); that kernel and vr_xcorr_argmax are not touched.  Nothing is accumulated with atomics
// and every reduction has a fixed order: two identical calls agree bit for bit.
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "model.h"

namespace vr {

namespace {

// sum over the workgroup (256 threads) in a fixed order -> every thread holds it
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double red[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                   // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// a larger correlation wins, an equal one at a lower index wins: np.argmax's first maximum, whatever the grid
__device__ __forceinline__ void lag_take(float& v, int& k, float ov, int ok) {
    if (ok >= 0 && (k < 0 || ov > v || (ov == v && ok < k))) { v = ov; k = ok; }
}

// -> thread 0 of the workgroup holds the workgroup's candidate
__device__ __forceinline__ void lag_reduce(float& v, int& k) {
    __shared__ float sv[4];
    __shared__ int sk[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_down(v, off, 64);
        const int ok = __shfl_down(k, off, 64);
        lag_take(v, k, ov, ok);
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; sk[threadIdx.x >> 6] = k; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) lag_take(v, k, sv[w], sk[w]);
}

}  // namespace

// The tiled lag search (XcorrTile).  full[k] = sum_n a[n + k - (nb - 1)] b[n] as xcorr_full_kernel states it, but a workgroup owns
// kLagTile = 512 consecutive lags and walks n in chunks of kLagChunk = 1024: the chunk of b and the kLagChunk + kLagTile samples of a that
// its lags meet go through LDS once (zero outside the heads, so no lag needs bounds of its own), each of the four waves takes a quarter of
// the chunk, and a lane keeps kLagR = 8 consecutive lags in registers: per four steps of n it reads one float4 of a (its window slides by
// four) and one float4 of b (the same address in every lane: a broadcast) for 32 multiply-adds.  The four waves' sums meet in LDS in a
// fixed order.  Its contract is the lag, not the bits of the correlation: the order of the additions differs from xcorr_full_kernel's.
template <class FORM>
__global__ __launch_bounds__(256) void xcorr_full_kernel(FORM f) {
    if constexpr (std::is_same<FORM, PrepRms>::value) {
        // grid (ceil(frames / 4), 2 channels, waves); one wave per frame: padded samples [f hop, f hop + frame) = original - frame / 2
        const PrepWave e = f.tab[blockIdx.z];
        const int fr = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (fr >= e.frames) return;                    // (a whole wave leaves: nothing below is workgroup-wide)
        const float* __restrict__ x = e.w + (long long)blockIdx.y * e.L;
        const long long j0 = (long long)fr * kTrimHop - kTrimFrame / 2;
        double s = 0.0;
#pragma unroll 4
        for (int i = 0; i < kTrimFrame / 64; ++i) {
            const long long j = j0 + i * 64 + lane;
            const double v = j >= 0 && j < e.L ? (double)x[j] : 0.0;
            s += v * v;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) e.rms[(long long)blockIdx.y * e.frames + fr] = (float)sqrt(s / (double)kTrimFrame);
    } else if constexpr (std::is_same<FORM, PrepTrim>::value) {
        // grid (waves); one workgroup per wave
        const PrepWave e = f.tab[blockIdx.x];
        if (!e.w) return;                              // (the absent second wave of a trim-only pair; uniform over the workgroup)
        __shared__ float smax[4];
        __shared__ int sfirst[4], slast[4];
        float ref = 0.f;
        for (int i = threadIdx.x; i < 2 * e.frames; i += 256) ref = fmaxf(ref, e.rms[i]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ref = fmaxf(ref, __shfl_xor(ref, off, 64));
        if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = ref;
        __syncthreads();
        ref = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
        // amplitude_to_db(ref=np.max, top_db=None) > -60 on any channel
        const double ref_db = 20.0 * log10((double)fmaxf(1e-5f, ref));
        int first = 0x7FFFFFFF, last = -1;
        for (int i = threadIdx.x; i < e.frames; i += 256) {
            const float r = fmaxf(e.rms[i], e.rms[e.frames + i]);                  // (log10 is monotone: the louder channel decides)
            if (20.0 * log10((double)fmaxf(1e-5f, r)) - ref_db > -60.0) {
                first = min(first, i);
                last = max(last, i);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            first = min(first, __shfl_xor(first, off, 64));
            last = max(last, __shfl_xor(last, off, 64));
        }
        if ((threadIdx.x & 63) == 0) { sfirst[threadIdx.x >> 6] = first; slast[threadIdx.x >> 6] = last; }
        __syncthreads();
        first = min(min(sfirst[0], sfirst[1]), min(sfirst[2], sfirst[3]));
        last = max(max(slast[0], slast[1]), max(slast[2], slast[3]));
        long long start = 0, end = 0;                  // no signal frame (a NaN wave): empty, as audio.trim
        if (last >= 0) {
            start = (long long)first * kTrimHop;
            end = (long long)(last + 1) * kTrimHop;
            if (end > e.L) end = e.L;
        }
        long long nh = end - start;
        if (nh > e.head_cap) nh = e.head_cap;
        const float* __restrict__ x0 = e.w + start;
        const float* __restrict__ x1 = e.w + e.L + start;
        double s = 0.0;
        for (long long j = threadIdx.x; j < nh; j += 256) s += (double)(x0[j] + x1[j]);
        s = block_sum(s);
        if (threadIdx.x == 0) *e.st = PrepState{start, end, nh, nh > 0 ? (float)(s / (double)nh) : 0.f, ref};
    } else if constexpr (std::is_same<FORM, PrepHeads>::value) {
        // grid (ceil(largest head / 256), waves)
        const PrepWave e = f.tab[blockIdx.y];
        if (!e.w) return;
        const PrepState st = *e.st;
        const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
        if (j < st.nh) e.head[j] = (e.w[st.start + j] + e.w[e.L + st.start + j]) - st.mean;
    } else if constexpr (std::is_same<FORM, XcorrTile>::value) {
        // grid (ceil((na + nb - 1) / kLagTile) for the largest heads the waves allow; a workgroup past the real count leaves)
        __shared__ alignas(16) float sa[kLagChunk + kLagTile];
        __shared__ alignas(16) float sb[kLagChunk];
        __shared__ float red[3][kLagTile];
        const long long na = f.p.sa->nh, nb = f.p.sb->nh;
        const long long nf = na + nb - 1;
        const long long k0 = (long long)blockIdx.x * kLagTile;
        if (na <= 0 || nb <= 0 || k0 >= nf) return;     // (uniform over the workgroup)
        const long long s0 = k0 - (nb - 1);            // shift of the block's first lag: lag k multiplies a[n + s0 + (k - k0)] by b[n]
        long long n_lo = -s0 - (kLagTile - 1), n_hi = na - s0;
        if (n_lo < 0) n_lo = 0;
        if (n_hi > nb) n_hi = nb;
        n_lo &= ~3LL;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const float* __restrict__ a = f.p.a;
        const float* __restrict__ b = f.p.b;
        float acc[kLagR];
#pragma unroll
        for (int r = 0; r < kLagR; ++r) acc[r] = 0.f;
        for (long long c0 = n_lo; c0 < n_hi; c0 += kLagChunk) {
            __syncthreads();
            for (int i = threadIdx.x; i < kLagChunk; i += 256) {
                const long long n = c0 + i;
                sb[i] = n < nb ? b[n] : 0.f;
            }
            for (int i = threadIdx.x; i < kLagChunk + kLagTile; i += 256) {
                const long long m = c0 + s0 + i;
                sa[i] = m >= 0 && m < na ? a[m] : 0.f;
            }
            __syncthreads();
            const int base = wave * (kLagChunk / 4);
            float win[kLagR + 4];
            {
                const float4 w0 = *reinterpret_cast<const float4*>(&sa[base + lane * kLagR]);
                const float4 w1 = *reinterpret_cast<const float4*>(&sa[base + lane * kLagR + 4]);
                win[0] = w0.x; win[1] = w0.y; win[2] = w0.z; win[3] = w0.w;
                win[4] = w1.x; win[5] = w1.y; win[6] = w1.z; win[7] = w1.w;
            }
#pragma unroll 2
            for (int i = base; i < base + kLagChunk / 4; i += 4) {
                const float4 nw = *reinterpret_cast<const float4*>(&sa[i + lane * kLagR + kLagR]);
                const float4 bb = *reinterpret_cast<const float4*>(&sb[i]);
                win[8] = nw.x; win[9] = nw.y; win[10] = nw.z; win[11] = nw.w;
                const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < kLagR; ++r) acc[r] = fmaf(win[u + r], bv[u], acc[r]);
#pragma unroll
                for (int r = 0; r < kLagR; ++r) win[r] = win[r + 4];
            }
        }
        if (wave > 0)
#pragma unroll
            for (int r = 0; r < kLagR; ++r) red[wave - 1][lane * kLagR + r] = acc[r];
        __syncthreads();
        if (wave == 0)
#pragma unroll
            for (int r = 0; r < kLagR; ++r) {
                const int q = lane * kLagR + r;
                if (k0 + q < nf) f.p.full[k0 + q] = ((acc[r] + red[0][q]) + red[1][q]) + red[2][q];
            }
    } else if constexpr (std::is_same<FORM, LagPart>::value) {
        // grid (kLagParts, pairs)
        const PrepPair p = f.tab[blockIdx.y];
        const long long na = p.sa->nh, nb = p.sb->nh;
        const long long nf = na > 0 && nb > 0 && !p.solo ? na + nb - 1 : 0;
        float v = 0.f;
        int k = -1;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nf; i += (long long)kLagParts * 256) {
            const float c = p.full[i];
            if (k < 0 || c > v) { v = c; k = (int)i; }     // (a thread meets its indices in rising order: the first of equals stays)
        }
        lag_reduce(v, k);
        if (threadIdx.x == 0) p.part[blockIdx.x] = LagCand{v, k};
    } else {
        static_assert(std::is_same<FORM, LagPick>::value, "xcorr_full_kernel: unknown form");
        // grid (pairs), one wave's worth of partials
        const PrepPair p = f.tab[blockIdx.x];
        float v = 0.f;
        int k = -1;
        if (threadIdx.x < kLagParts) { const LagCand c = p.part[threadIdx.x]; v = c.v; k = c.k; }
        lag_reduce(v, k);
        if (threadIdx.x == 0) {
            const PrepState sa = *p.sa, sb = *p.sb;
            PairWindow w{sa.start, sa.end, sb.start, sb.end, k < 0 ? 0 : (long long)k - (sa.nh - 1), 0, 0, 0};
            *p.out = w;
        }
    }
}

void launch_prep_trim(const PrepWave* tab_dev, int n_waves, int max_frames, long long max_head, hipStream_t st) {
    VR_LAUNCH(xcorr_full_kernel<PrepRms>, dim3((unsigned)((max_frames + 3) / 4), 2, (unsigned)n_waves), dim3(256), 0, st, PrepRms{tab_dev});
    VR_HIP(hipGetLastError());
    VR_LAUNCH(xcorr_full_kernel<PrepTrim>, dim3((unsigned)n_waves), dim3(256), 0, st, PrepTrim{tab_dev});
    VR_HIP(hipGetLastError());
    VR_LAUNCH(xcorr_full_kernel<PrepHeads>, dim3((unsigned)((max_head + 255) / 256), (unsigned)n_waves), dim3(256), 0, st, PrepHeads{tab_dev});
    VR_HIP(hipGetLastError());
}

void launch_xcorr_tile(const PrepPair& p, long long nf_max, hipStream_t st) {
    prof_note(0.0, 4.0 * 3.0 * (double)nf_max);
    VR_LAUNCH(xcorr_full_kernel<XcorrTile>, dim3((unsigned)((nf_max + kLagTile - 1) / kLagTile)), dim3(256), 0, st, XcorrTile{p});
    VR_HIP(hipGetLastError());
}

void launch_lag_argmax(const PrepPair* tab_dev, int n_pairs, hipStream_t st) {
    VR_LAUNCH(xcorr_full_kernel<LagPart>, dim3(kLagParts, (unsigned)n_pairs), dim3(256), 0, st, LagPart{tab_dev});
    VR_HIP(hipGetLastError());
    VR_LAUNCH(xcorr_full_kernel<LagPick>, dim3((unsigned)n_pairs), dim3(256), 0, st, LagPick{tab_dev});
    VR_HIP(hipGetLastError());
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
    char* bytes(size_t n) {
        const size_t a = (off + 255) & ~size_t(255);
        off = a + n;
        return base ? base + a : nullptr;
    }
    template <class T>
    T* of(size_t n) { return reinterpret_cast<T*>(bytes(n * sizeof(T))); }
};

std::string pair_name(int i) { return "pair " + std::to_string(i); }

}  // namespace

// Everything that can be said of the arguments without a device (the C entry calls this first, then looks for the device).
void align_pair_check(int n, const float* const* mix, const float* const* inst, const long long* L_mix, const long long* L_inst, int sr,
                      const void* out) {
    VR_CHECK(n > 0 && mix && inst && L_mix && L_inst && out, -2, "align pair: no pair or a null table");
    VR_CHECK(n <= 32767, -2, "align pair: at most 32767 pairs in one call (one grid plane per wave)");
    VR_CHECK(sr > 0 && sr <= (1 << 27), -2, "align pair: the sample rate must be positive (and at most 2^27: the 'full' correlation is indexed in int32)");
    for (int i = 0; i < n; ++i) {
        VR_CHECK(mix[i], -2, "align pair: " + pair_name(i) + ": null mixture");
        VR_CHECK(L_mix[i] > 0 && (!inst[i] || L_inst[i] > 0), -2, "align pair: " + pair_name(i) + ": empty wave");
        VR_CHECK(L_mix[i] < (1LL << 38) && (!inst[i] || L_inst[i] < (1LL << 38)), -2, "align pair: " + pair_name(i) + ": wave too long");
    }
}

void align_pair_many_api(int device, int n, const float* const* mix, const float* const* inst, bool on_dev, const long long* L_mix,
                         const long long* L_inst, int sr, PairWindow* out) {
    align_pair_check(n, mix, inst, L_mix, L_inst, sr, out);
    for (int i = 0; on_dev && i < n; ++i)
        VR_CHECK(((reinterpret_cast<uintptr_t>(mix[i]) | reinterpret_cast<uintptr_t>(inst[i])) & 3) == 0, -2,
                 "align pair: " + pair_name(i) + ": a device wave must be 4-byte aligned");
    DeviceGuard dev_guard(device);
    const long long head_cap = 4LL * sr;
    const int W = 2 * n;
    std::vector<PrepWave> tab((size_t)W);
    std::vector<PrepPair> pairs((size_t)n);
    int max_frames = 0;
    long long max_head = 0;
    DevBuf buf;
    // the same carve twice: once for the total, once for the pointers
    for (int pass = 0; pass < 2; ++pass) {
        Carve c(buf.p);
        PrepWave* tab_dev = c.of<PrepWave>((size_t)W);
        PrepPair* pair_dev = c.of<PrepPair>((size_t)n);
        PrepState* st_dev = c.of<PrepState>((size_t)W);
        PairWindow* win_dev = c.of<PairWindow>((size_t)n);
        for (int i = 0; i < n; ++i) {
            const bool solo = inst[i] == nullptr;           // trim only: the second entry stays empty and no kernel reads it
            for (int s = 0; s < (solo ? 1 : 2); ++s) {
                PrepWave& e = tab[2 * i + s];
                e.L = s ? L_inst[i] : L_mix[i];
                e.head_cap = head_cap;
                e.frames = 1 + (int)(e.L / kTrimHop);
                const float* src = s ? inst[i] : mix[i];
                float* stage = on_dev ? nullptr : c.of<float>((size_t)2 * e.L);
                e.w = on_dev ? src : stage;
                e.rms = c.of<float>((size_t)2 * e.frames);
                e.head = c.of<float>((size_t)std::min(head_cap, e.L));
                e.st = st_dev + (2 * i + s);
                max_frames = std::max(max_frames, e.frames);
                max_head = std::max(max_head, std::min(head_cap, e.L));
            }
            PrepPair& p = pairs[i];
            p.solo = solo ? 1 : 0;
            p.sa = st_dev + 2 * i; p.sb = solo ? p.sa : st_dev + 2 * i + 1;
            p.a = tab[2 * i].head; p.b = solo ? p.a : tab[2 * i + 1].head;
            p.full = solo ? nullptr : c.of<float>((size_t)(std::min(head_cap, L_mix[i]) + std::min(head_cap, L_inst[i]) - 1));
            p.part = c.of<LagCand>(kLagParts);
            p.out = win_dev + i;
        }
        if (pass == 1) {
            hipStream_t st = nullptr;
            if (!on_dev)
                for (int i = 0; i < n; ++i)
                    for (int s = 0; s < (inst[i] ? 2 : 1); ++s)
                        VR_HIP(hipMemcpyAsync(const_cast<float*>(tab[2 * i + s].w), s ? inst[i] : mix[i], (size_t)2 * tab[2 * i + s].L * sizeof(float),
                                              hipMemcpyHostToDevice, st));
            VR_HIP(hipMemcpyAsync(tab_dev, tab.data(), (size_t)W * sizeof(PrepWave), hipMemcpyHostToDevice, st));
            VR_HIP(hipMemcpyAsync(pair_dev, pairs.data(), (size_t)n * sizeof(PrepPair), hipMemcpyHostToDevice, st));
            launch_prep_trim(tab_dev, W, max_frames, max_head, st);
            for (int i = 0; i < n; ++i)
                if (!pairs[i].solo) launch_xcorr_tile(pairs[i], std::min(head_cap, L_mix[i]) + std::min(head_cap, L_inst[i]) - 1, st);
            launch_lag_argmax(pair_dev, n, st);
            VR_HIP(hipMemcpyAsync(out, win_dev, (size_t)n * sizeof(PairWindow), hipMemcpyDeviceToHost, st));
            VR_HIP(hipStreamSynchronize(st));
            break;
        }
        const size_t need = c.off + 256;
        if (hipMalloc(reinterpret_cast<void**>(&buf.p), need) != hipSuccess) {
            (void)hipGetLastError();
            buf.p = nullptr;
            throw Error(-4, "align pair: hipMalloc of " + std::to_string(need) + " bytes of workspace failed (" + std::to_string(n) +
                                " pairs" + (on_dev ? "" : ", their waves staged on the device") + ")");
        }
    }
    for (int i = 0; i < n; ++i)
        VR_CHECK(pair_window_plan(out[i]), -2,
                 "align pair: " + pair_name(i) + ": the common window is empty (trimmed mixture [" + std::to_string(out[i].a_start) + ", " +
                     std::to_string(out[i].a_end) + "), instrumental [" + std::to_string(out[i].b_start) + ", " + std::to_string(out[i].b_end) +
                     "), lag " + std::to_string(out[i].lag) + ")");
}

// vr_pair_rows_many.  The items follow each other on the handle's stream through one workspace sized for the largest pair: the two
// windows [2][n] and, for host outputs, the two row blocks; the peak candidates of every pair stay until the one wait of the call.
void Model::pair_rows_run(int n, const float* const* mix, const float* const* inst, bool on_dev, const long long* L_mix, const long long* L_inst,
                          const PairWindow* w, long long max_bytes, float* const* X_out, float* const* y_out, bool out_on_dev, float* peaks) {
    const std::string who = "pair rows: ";
    VR_CHECK(n > 0 && mix && inst && L_mix && L_inst && w && X_out && y_out && peaks, -2, who + "no pair or a null table");
    VR_CHECK(istft_masked_available(plan, hop), -9,
             who + "the rows are a form of the frame-tiled STFT, which this handle does not have (hop_length == n_fft / 2 needed): take the "
                   "host route, two vr_stft calls");
    size_t item = 0;
    for (int i = 0; i < n; ++i) {
        VR_CHECK(mix[i] && inst[i] && X_out[i] && y_out[i], -2, who + pair_name(i) + ": null wave or output");
        VR_CHECK(w[i].n > 0 && w[i].a_off >= 0 && w[i].b_off >= 0 && w[i].a_off <= L_mix[i] - w[i].n && w[i].b_off <= L_inst[i] - w[i].n, -2,
                 who + pair_name(i) + ": the window (" + std::to_string(w[i].n) + " samples from " + std::to_string(w[i].a_off) + " / " +
                     std::to_string(w[i].b_off) + ") leaves its waves of " + std::to_string(L_mix[i]) + " / " + std::to_string(L_inst[i]) + " samples");
        VR_CHECK(w[i].n / hop < (1LL << 28), -2, who + pair_name(i) + ": window too long");
        // the peak kernel reads the rows as float4, the copies read the waves as float
        VR_CHECK(!out_on_dev || ((reinterpret_cast<uintptr_t>(X_out[i]) | reinterpret_cast<uintptr_t>(y_out[i])) & 15) == 0, -2,
                 who + pair_name(i) + ": a device output must be 16-byte aligned");
        VR_CHECK(!on_dev || ((reinterpret_cast<uintptr_t>(mix[i]) | reinterpret_cast<uintptr_t>(inst[i])) & 3) == 0, -2,
                 who + pair_name(i) + ": a device wave must be 4-byte aligned");
        const size_t rows_f = (size_t)(1 + w[i].n / hop) * 2 * output_bin * 2;
        Carve c(nullptr);
        c.of<float>((size_t)2 * w[i].n); c.of<float>((size_t)2 * w[i].n);
        if (!out_on_dev) { c.of<float>(rows_f); c.of<float>(rows_f); }
        item = std::max(item, c.off);
    }
    const size_t peak_b = (size_t)(kPeakParts + 1) * sizeof(PeakCand);
    const size_t need = item + 256 + (size_t)n * (peak_b + 256);
    DeviceGuard dev_guard(device);
    size_t budget = 0;
    if (max_bytes > 0) budget = (size_t)max_bytes;
    else {
        size_t free_b = 0, total_b = 0;
        VR_HIP(hipMemGetInfo(&free_b, &total_b));
        budget = free_b - free_b / 10;
    }
    VR_CHECK(need <= budget, -4, who + "the largest pair needs " + std::to_string(need) + " bytes of device workspace (" + std::to_string(need >> 20) +
                                 " MiB: its two windows" + (out_on_dev ? "" : " and their rows") + "), the budget allows " + std::to_string(budget) +
                                 (max_bytes > 0 ? " (max_bytes)" : " (nine tenths of the free device memory)"));
    DevBuf buf;
    if (hipMalloc(reinterpret_cast<void**>(&buf.p), need) != hipSuccess) {
        (void)hipGetLastError();
        buf.p = nullptr;
        throw Error(-4, who + "hipMalloc of " + std::to_string(need) + " bytes of workspace failed");
    }
    const hipMemcpyKind in_kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    std::vector<PeakCand> cand((size_t)n);
    std::vector<PeakCand*> cand_dev((size_t)n);
    {
        Carve c(buf.p);
        c.bytes(item);
        for (int i = 0; i < n; ++i) cand_dev[i] = reinterpret_cast<PeakCand*>(c.bytes(peak_b));
    }
    for (int i = 0; i < n; ++i) {
        const long long len = w[i].n;
        const int T = 1 + (int)(len / hop);
        const size_t rows_f = (size_t)T * 2 * output_bin * 2;
        Carve c(buf.p);
        float* wa = c.of<float>((size_t)2 * len);
        float* wb = c.of<float>((size_t)2 * len);
        float* rx = out_on_dev ? X_out[i] : c.of<float>(rows_f);
        float* ry = out_on_dev ? y_out[i] : c.of<float>(rows_f);
        const size_t row_b = (size_t)len * sizeof(float);
        VR_HIP(hipMemcpy2DAsync(wa, row_b, mix[i] + w[i].a_off, (size_t)L_mix[i] * sizeof(float), row_b, 2, in_kind, stream));
        VR_HIP(hipMemcpy2DAsync(wb, row_b, inst[i] + w[i].b_off, (size_t)L_inst[i] * sizeof(float), row_b, 2, in_kind, stream));
        launch_stft_rows(plan, wa, len, T, reinterpret_cast<float2*>(rx), stream);
        launch_stft_rows(plan, wb, len, T, reinterpret_cast<float2*>(ry), stream);
        const long long elems = (long long)T * 2 * output_bin;
        launch_song_peak(reinterpret_cast<const float2*>(rx), reinterpret_cast<const float2*>(ry), elems, cand_dev[i], stream);
        VR_HIP(hipMemcpyAsync(&cand[i], cand_dev[i] + song_peak_parts(elems), sizeof(PeakCand), hipMemcpyDeviceToHost, stream));
        if (!out_on_dev) {
            VR_HIP(hipMemcpyAsync(X_out[i], rx, rows_f * sizeof(float), hipMemcpyDeviceToHost, stream));
            VR_HIP(hipMemcpyAsync(y_out[i], ry, rows_f * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
    }
    // one wait for the call: the stream orders every reuse of the workspace
    VR_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i) peaks[i] = cand[i].bad ? std::numeric_limits<float>::quiet_NaN() : numpy_cabsf(cand[i].re, cand[i].im);
}

}  // namespace vr
