// STFT / iSTFT and the spectrogram-side glue of inference.Separator, all device-resident.
//
//  K1  stft         : librosa.stft semantics at the reference call site lib/spec_utils.py:26-31
//                     (periodic Hann, centre zero-padding n_fft/2, frames 1 + L//hop, complex64).
//  K2  mag_pad      : |X| into the zero-padded crop source + the two normalisers the reference
//                     uses (inference.py:74 max|X|; inference.py:87,94 numpy's lexicographic
//                     complex max).
//  K14 istft        : librosa.istft at lib/spec_utils.py:157-165 (irfft * window, overlap-add,
//                     / window-sum-square where > tiny, trim n_fft/2) -> hop*(T-1) samples.
//      apply_mask   : inference.py:26-40 (y = mask*X, v = (1-mask)*X; TTA average :97-98).
//      <true> forms : the complex-mask model (CascadedNet(is_complex=True)): the complex input pack
//                     (mag_pad), the complex normaliser (coef_affine) and the consumers of a complex64 mask.
// One workgroup per frame; radix-2 FFT in LDS.  These stages are HBM-bound streaming work that is
// <1 % of the pipeline, kept simple and exact-ordered.
#include "kernels.h"
#include "pcm.h"

#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace vr {

// The kernels of the spectrogram side exist in two forms under one name.  SRC = const float2 (the default): one song, every
// argument as documented at the kernel.  SRC = const SongSeg (vr_separate_many / vr_separate_wave_many): `src` is the call's song
// table and one more grid dimension picks the song; the kernel takes that song's pointers, length and mask columns from its entry
// and then runs the same code.  `mask_a` is then the call's concatenated mask (row pitch Wa), `mask_b` the same pointer when the TTA
// pass is to be averaged in (else null), `wgt` the weights of all songs; the arguments an entry replaces are passed as 0.
template <class SRC> constexpr bool kSongTable = std::is_same<SRC, const SongSeg>::value;
// SRC = const StreamSeg (vr_stream_*): `src` is a table of StreamSeg, one entry per stream taking a step (vr_stream_push: one entry), and
// one more grid dimension picks the entry, as for the song table.  Frames and samples are addressed by their absolute index in the
// stream and live in rings (kernels.h); each kernel handles only what the step added to its entry's stream.
template <class SRC> constexpr bool kStream = std::is_same<SRC, const StreamSeg>::value;
template <class SRC> using StreamLocal = typename std::conditional<kStream<SRC>, StreamSeg, int>::type;
// SRC = const WavePair (the wave-domain loss term): `src` is one WavePair in device memory and blockIdx.y runs over
// its signals; the workgroup runs its frame tile twice, for the target and for the estimate (kernels.h).
template <class SRC> constexpr bool kPair = std::is_same<SRC, const WavePair>::value;
template <class SRC> using PairLocal = typename std::conditional<kPair<SRC>, WavePair, int>::type;
// SRC = const WaveTriple (the weighted SDR term): the same with three passes -- the mixture, the target, the estimate.
template <class SRC> constexpr bool kTriple = std::is_same<SRC, const WaveTriple>::value;
template <class SRC> using TripleLocal = typename std::conditional<kTriple<SRC>, WaveTriple, int>::type;
// SRC = const CropSeg (the wave store of vr_dataset_*): `src` is a table with one entry per signal and blockIdx.z picks
// the entry; the workgroup computes frames of that entry's own wave, counted from the entry's first row, and stores them as rows.
template <class SRC> constexpr bool kCrops = std::is_same<SRC, const CropSeg>::value;
template <class SRC> using CropLocal = typename std::conditional<kCrops<SRC>, CropSeg, int>::type;

// sample p of channel ch of a stream: the tail kept from earlier steps, then the step's block; zero outside [0, L)
__device__ __forceinline__ float stream_sample(const StreamSeg& sg, int ch, long long p) {
    if (p < 0 || p >= sg.L) return 0.f;
    return p < sg.blk_base ? sg.tail[(long long)ch * sg.tail_pitch + (p - sg.tail_base)] : sg.blk[(long long)ch * sg.blk_pitch + (p - sg.blk_base)];
}
// the same where the step's block is sample bytes (`in`: the entry's PcmIn, whose bytes begin at the block's first frame): the tail is
// float, kept per network channel `ch`; the block is read through pcm_decode at the file's channel in.ch
template <class IN>
__device__ __forceinline__ float stream_sample_pcm(const StreamSeg& sg, const IN& in, int ch, long long p) {
    if (p < 0 || p >= sg.L) return 0.f;
    return p < sg.blk_base ? sg.tail[(long long)ch * sg.tail_pitch + (p - sg.tail_base)] : in.at(p - sg.blk_base);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// a - b and a + b per component, each one float32 operation of its own: never contracted with a product on either side, so that the
// result is numpy's complex64 difference / sum of the two rounded values (the pseudo-label forms)
__device__ __forceinline__ float2 sub_rounded(float2 a, float2 b) {
#pragma clang fp contract(off)
    return make_float2(a.x - b.x, a.y - b.y);
}
__device__ __forceinline__ float2 add_rounded(float2 a, float2 b) {
#pragma clang fp contract(off)
    return make_float2(a.x + b.x, a.y + b.y);
}

// In-place radix-2 DIT FFT on x[0..n) (already in bit-reversed order). tw[k] = exp(-2*pi*i*k/n).
__device__ __forceinline__ void fft_lds(float2* x, const float2* __restrict__ tw, int n, int log2n) {
    const int half_n = n >> 1;
    for (int s = 0; s < log2n; ++s) {
        const int half = 1 << s;
        __syncthreads();
        for (int b = threadIdx.x; b < half_n; b += blockDim.x) {
            const int pos = b & (half - 1);
            const int i = ((b >> s) << (s + 1)) + pos;
            const int j = i + half;
            const float2 w = tw[pos << (log2n - 1 - s)];
            const float2 t = cmul(w, x[j]);
            const float2 u = x[i];
            x[i] = make_float2(u.x + t.x, u.y + t.y);
            x[j] = make_float2(u.x - t.x, u.y - t.y);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void stft_kernel(FFTPlan pl, const float* __restrict__ wave, long long L,
                                                   int hop, int T, float2* __restrict__ spec) {
    extern __shared__ __attribute__((aligned(16))) float2 xs[];
    const int n = pl.n_fft, t = blockIdx.x, ch = blockIdx.y;
    const float* wv = wave + (long long)ch * L;
    const long long start = (long long)t * hop - n / 2;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const long long p = start + i;
        const float v = (p >= 0 && p < L) ? wv[p] * pl.window[i] : 0.f;
        const int r = __brev((unsigned)i) >> (32 - pl.log2n);
        xs[r] = make_float2(v, 0.f);
    }
    fft_lds(xs, pl.twiddle, n, pl.log2n);
    const int bins = n / 2 + 1;
    for (int k = threadIdx.x; k < bins; k += blockDim.x)
        spec[((long long)ch * bins + k) * T + t] = xs[k];
}

void launch_stft(const FFTPlan& pl, const float* wave, long long L, int hop, int T, float2* spec, hipStream_t st);
static int tile_frames(const FFTPlan& pl, int extra_floats);
static bool tiled_signal_path(const FFTPlan& pl, int hop);
void launch_stft_tiled(const FFTPlan& pl, const float* wave, long long L, int T, float2* spec, hipStream_t st);

void launch_stft(const FFTPlan& pl, const float* wave, long long L, int hop, int T, float2* spec, hipStream_t st) {
    if (tiled_signal_path(pl, hop)) { launch_stft_tiled(pl, wave, L, T, spec, st); return; }
    VR_LAUNCH(stft_kernel, dim3(T, 2), dim3(256), pl.n_fft * sizeof(float2), st, pl, wave, L, hop, T, spec);
    VR_HIP(hipGetLastError());
}

// =====================================================================================================
// Frame-tiled STFT / iSTFT for hop == n_fft/2 (every reference call site: n_fft 2048, hop 1024).
//
// One workgroup = F consecutive frames of one channel.  Each frame is ONE n_fft/2-point complex FFT of the packed real
// signal z[m] = x[2m] + i x[2m+1]; the spectrum is unpacked with E[k] = (Z[k] + conj Z[M-k]) / 2,
// O[k] = -i (Z[k] - conj Z[M-k]) / 2, X[k] = E[k] + e^{-2 pi i k / N} O[k].  The F spectra are collected in an LDS tile
// [bins][F] and written as rows of F complex values (128 B for F = 16): the reference layout [ch][bins][T] is stored
// coalesced instead of one 8-byte element per 10 KB stride (measured before: 4.3x the algorithmic write traffic).
// The inverse reads the same tiles (optionally times the mask: inference.py:26-40 fused into the load), runs the packed
// inverse FFT, applies the window and overlap-adds inside the workgroup (hop = n_fft/2: a sample = second half of frame s
// + first half of frame s+1), so the [ch][T][n_fft] frame buffer and its 13x gather traffic are gone.
// =====================================================================================================
// radix-2 DIT on n points (bit-reversed input) by the `nt` threads of one frame group (tid = 0..nt-1); tw is the table
// of a 2^twshift times larger transform.  Barriers are workgroup-wide: every group runs the same number of stages.
__device__ __forceinline__ void fft_lds_sub(float2* x, const float2* __restrict__ tw, int n, int log2n, int twshift, int tid,
                                            int nt) {
    const int half_n = n >> 1;
    for (int s = 0; s < log2n; ++s) {
        const int half = 1 << s;
        __syncthreads();
        for (int b = tid; b < half_n; b += nt) {
            const int pos = b & (half - 1);
            const int i = ((b >> s) << (s + 1)) + pos;
            const int j = i + half;
            const float2 w = tw[(pos << (log2n - 1 - s)) << twshift];
            const float2 t = cmul(w, x[j]);
            const float2 u = x[i];
            x[i] = make_float2(u.x + t.x, u.y + t.y);
            x[j] = make_float2(u.x - t.x, u.y - t.y);
        }
    }
    __syncthreads();
}

constexpr int TG = 4;                        // frames in flight per workgroup (1024 threads = 4 groups of 256)

template <class A> __device__ __forceinline__ A pcm_first(A a) { return a; }
// the first type of a pack, or D for an empty one: the format arguments of the tile kernels are trailing packs, so that an instantiation
// without one keeps its signature and its name (the launch profiler's report and the tests that read it know the kernels by name)
template <class D, class... T> struct FirstOr { using type = D; };
template <class D, class A, class... T> struct FirstOr<D, A, T...> { using type = A; };

// Where the STFT fetches sample p of its channel, and where the iSTFT stores sample p + i of channel ch: the file's sample format is a
// template argument of the two tile kernels, not a pass of its own (csrc/pcm.h holds the arithmetic).
struct WaveF32In {                           // planar float32 [2][L]: the channel's row
    const float* wv;
    __device__ __forceinline__ float at(long long p) const { return wv[p]; }
};
struct WavePcmIn {                           // interleaved frames of 1 or 2 channels in a WAV sample format; a mono file is up-mixed
    PcmIn in;
    int ch;
    __device__ __forceinline__ float at(long long p) const { return pcm_decode(in.bytes, in.fmt, in.channels, p, ch); }
};
struct WaveCropIn {                          // a crop-table entry's wave: planar float32 (fmt 0) or the file's sample bytes
    WaveF32In f;
    WavePcmIn p;
    int fmt;
    __device__ __forceinline__ float at(long long i) const { return fmt ? p.at(i) : f.at(i); }
};
struct WaveGradIn {                          // the wave gradient of the SDR term over the iSTFT's envelope: (alpha y + beta p)[p] / env(p)
    const float* yw;
    const float* pw;
    const float* win;
    float alpha, beta;
    int M;
    __device__ __forceinline__ float at(long long p) const {
        const int i = (int)(p & (M - 1));
        const float w0 = win[i], w2 = win[i + M];
        const float ws = fmaf(w0, w0, w2 * w2);      // the envelope istft_tile_kernel divides by (and its guard)
        const float a = fmaf(alpha, yw[p], beta * pw[p]);
        return ws > FLT_MIN ? a / ws : a;
    }
};
struct WaveGrad3In {                         // the same for the weighted SDR term: (cy y + cp p + cx x)[p] / env(p)
    const float* xw;
    const float* yw;
    const float* pw;
    const float* win;
    float cy, cp, cx;
    int M;
    __device__ __forceinline__ float at(long long p) const {
        const int i = (int)(p & (M - 1));
        const float w0 = win[i], w2 = win[i + M];
        const float ws = fmaf(w0, w0, w2 * w2);
        const float a = fmaf(cy, yw[p], fmaf(cp, pw[p], cx * xw[p]));
        return ws > FLT_MIN ? a / ws : a;
    }
};
struct WaveF32Out {                          // planar float32 [2][pitch]
    static constexpr bool kInterleaved = false;
    static __device__ __forceinline__ void put(float* w, long long pitch, int ch, long long p, int i, float v) { w[(long long)ch * pitch + p + i] = v; }
};
struct WavePcm16Out {                        // interleaved int16 [samples][2] behind the kernel's float pointer
    static constexpr bool kInterleaved = true;
    static __device__ __forceinline__ void put(float* w, long long, int ch, long long p, int i, float v) {
        reinterpret_cast<int16_t*>(w)[(p + i) * 2 + ch] = pcm16_from_float(v);
    }
};

// PCM (at most one type): none = `wave` / the song table's `wave` are planar float32, as documented above.  PcmIn (SRC = const float, `wave`
// unused) = the call's interleaved sample bytes; const PcmIn* (SRC = const SongSeg) = one entry per song beside the song table, whose
// `wave` pointers are then unused; const PcmIn* (SRC = const StreamSeg) = one entry per table entry beside the stream
// table: the step's block (`blk`, then unused) is that entry's interleaved sample bytes from the block's first frame on, format and channel
// count per entry.  The input tail stays float32: `tail_out` receives the decoded samples, so the next step, float or PCM, reads the floats
// a float push would have left.
// WaveGrad in the same place (SRC = const float, `wave` and `spec` unused): the adjoint of the inverse transform for the wave-domain loss
// term (kernels.h) -- blockIdx.y runs over the signals, L = hop (T-1), the source is WaveGradIn and the store epilogue writes dmask.
// WaveGrad3: the same for the weighted SDR term, source WaveGrad3In over three waves, the same store epilogue.
// SpecRows (SRC = const float): the same spectrogram stored as rows [T][2][bins], the training cache's layout.
// const PseudoSeg* (SRC = const SongSeg): the pair form -- one PseudoSeg per song beside the song table.  The workgroup
// runs its frame tile twice with the same arithmetic: first the song's instrumental (`inst_wave`), stored to `inst` as vr_stft stores it,
// then the table's mixture, of which only D = X - Y goes to the table's `spec`; X itself is never written.
// SRC = const CropSeg (no PCM type): the crop-table form -- blockIdx.z picks the entry, frame f of the grid is row
// start + f of the entry's wave (the samples are checked against the wave's own n, so row 0 and the last rows meet the zero padding they
// meet in the whole song's transform), the entry's fmt picks the reader, and the rows go to the entry's dst as the SpecRows form stores them.
template <class SRC = const float, class... PCM>
__global__ __launch_bounds__(1024) void stft_tile_kernel(FFTPlan pl, SRC* __restrict__ wave, long long L, int T, int F,
                                                         float2* __restrict__ spec, PCM... pcm) {
    constexpr bool kGrad3 = std::is_same<typename FirstOr<void, PCM...>::type, WaveGrad3>::value;
    constexpr bool kGrad = std::is_same<typename FirstOr<void, PCM...>::type, WaveGrad>::value || kGrad3;
    constexpr bool kPseudo = std::is_same<typename FirstOr<void, PCM...>::type, const PseudoSeg*>::value;
    constexpr bool kRows = std::is_same<typename FirstOr<void, PCM...>::type, SpecRows>::value;
    constexpr bool kPcm = sizeof...(PCM) == 1 && !kGrad && !kPseudo && !kRows;
    static_assert(!kPseudo || kSongTable<SRC>, "the pair form is a song-table form");
    static_assert(!kRows || std::is_same<SRC, const float>::value, "the rows form is a one-song form");
    static_assert(!kCrops<SRC> || sizeof...(PCM) == 0, "a crop entry names its own sample format");
    static_assert(sizeof...(PCM) <= 1, "one PCM source at most");
    static_assert(!kStream<SRC> || sizeof...(PCM) == 0 || std::is_same<typename FirstOr<void, PCM...>::type, const PcmIn*>::value,
                  "a stream's PCM source is a table of PcmIn beside the stream table");
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int n = pl.n_fft, M = n >> 1, bins = M + 1, hop = M, logM = pl.log2n - 1;
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    float2* zs = lds2 + (size_t)g * M;       // this group's FFT buffer
    float2* tile = lds2 + (size_t)TG * M;    // [bins][F]
    int t0 = blockIdx.x * F;
    const int ch = blockIdx.y;
    typename std::conditional<kCrops<SRC>, WaveCropIn, typename std::conditional<kPcm, WavePcmIn, typename std::conditional<kGrad3, WaveGrad3In,
                              typename std::conditional<kGrad, WaveGradIn, WaveF32In>::type>::type>::type>::type in;
    CropLocal<SRC> cs{};
    typename std::conditional<kGrad3, WaveGrad3, typename std::conditional<kGrad, WaveGrad, int>::type>::type gd{};
    StreamLocal<SRC> ss{};
    typename std::conditional<kPseudo, PseudoSeg, int>::type ps{};
    const float* mix_wv = nullptr;                   // (pseudo) the mixture's row, for pass 1
    if constexpr (kStream<SRC>) {                    // blockIdx.z = table entry; the frames [t_new, T) of its stream, written into the ring
        ss = wave[blockIdx.z];
        if (blockIdx.x > 0 && t0 >= ss.T - ss.t_new) return;        // (workgroup 0 always runs: it moves the input tail on)
        t0 += ss.t_new; T = ss.T;
        if constexpr (kPcm) in.in = pcm_first(pcm...)[blockIdx.z];
        else in.wv = nullptr;
    } else if constexpr (kSongTable<SRC>) {          // blockIdx.z = song; the grid is sized for the longest one
        const SongSeg sg = wave[blockIdx.z];
        if (t0 >= sg.T) return;
        L = sg.L; T = sg.T; spec = sg.spec;
        if constexpr (kPcm) in.in = pcm_first(pcm...)[blockIdx.z];
        else in.wv = sg.wave + (long long)ch * L;
        if constexpr (kPseudo) {
            ps = pcm_first(pcm...)[blockIdx.z];
            mix_wv = in.wv;
            in.wv = ps.inst_wave + (long long)ch * L;
        }
    } else if constexpr (kCrops<SRC>) {              // blockIdx.z = entry; the grid is sized for the longest crop
        cs = wave[blockIdx.z];
        if (t0 >= cs.T) return;
        L = cs.n; T = cs.T; spec = cs.dst;
        in.fmt = cs.fmt;
        in.f.wv = static_cast<const float*>(cs.wave) + (long long)ch * L;
        in.p.in = PcmIn{static_cast<const uint8_t*>(cs.wave), cs.channels, cs.fmt};
        in.p.ch = ch < cs.channels ? ch : cs.channels - 1;
    } else if constexpr (kGrad3) {                   // cy, cp, cx from the six batch-wide sums the triple iSTFT left in device memory
        gd = pcm_first(pcm...);
        const WsdrCoef c = wsdr_coefficients((double)gd.sums[0], (double)gd.sums[1], (double)gd.sums[2], (double)gd.sums[3],
                                             (double)gd.sums[4], (double)gd.sums[5]);
        in.xw = gd.x_wave + (long long)ch * L; in.yw = gd.y_wave + (long long)ch * L; in.pw = gd.p_wave + (long long)ch * L;
        in.win = pl.window; in.M = M;
        in.cy = (float)((double)gd.sdr_scale * c.cy); in.cp = (float)((double)gd.sdr_scale * c.cp); in.cx = (float)((double)gd.sdr_scale * c.cx);
    } else if constexpr (kGrad) {                    // alpha, beta from the batch-wide sums the pair iSTFT left in device memory
        gd = pcm_first(pcm...);
        const double a = (double)gd.sums[0], p = sqrt((double)gd.sums[1]), q = sqrt((double)gd.sums[2]), D = p * q + 1e-8;
        in.yw = gd.y_wave + (long long)ch * L; in.pw = gd.p_wave + (long long)ch * L; in.win = pl.window; in.M = M;
        in.alpha = (float)(-(double)gd.sdr_scale / D);
        in.beta = q > 0.0 ? (float)((double)gd.sdr_scale * a * p / (q * D * D)) : 0.f;
    } else {
        if constexpr (kPcm) in.in = pcm_first(pcm...);
        else in.wv = wave + (long long)ch * L;
    }
    if constexpr (kPcm) in.ch = ch < in.in.channels ? ch : in.in.channels - 1;
    const int nf = (T - t0) < F ? (T - t0) : F;
    // (pseudo) pass 0 = the instrumental Y, stored as it is; pass 1 = the mixture X, of which only D = X - Y is stored: a thread unpacks the
    // same (bin, frame) elements in both passes, so pass 1 reads back its own tile entries.  (A jump back, not a loop around the body:
    // every other form then has no loop in its source and keeps the code it had.)
    int pass = 0;
second_pass:
    for (int f0 = 0; f0 < nf; f0 += TG) {
        const int f = f0 + g;
        const bool live = f < nf;
        if (live) {
            long long start = (long long)(t0 + f) * hop - M;            // centre = True: n_fft/2 zeros in front
            if constexpr (kCrops<SRC>) start += cs.start * hop;         // (frame f of a crop is row start + f of its song)
            for (int m = tid; m < M; m += 256) {
                const long long p = start + 2 * m;
                float v0, v1;
                if constexpr (kStream<SRC> && kPcm) {
                    v0 = stream_sample_pcm(ss, in, ch, p) * pl.window[2 * m];
                    v1 = stream_sample_pcm(ss, in, ch, p + 1) * pl.window[2 * m + 1];
                } else if constexpr (kStream<SRC>) {
                    v0 = stream_sample(ss, ch, p) * pl.window[2 * m];
                    v1 = stream_sample(ss, ch, p + 1) * pl.window[2 * m + 1];
                } else {
                    v0 = (p >= 0 && p < L) ? in.at(p) * pl.window[2 * m] : 0.f;
                    v1 = (p + 1 >= 0 && p + 1 < L) ? in.at(p + 1) * pl.window[2 * m + 1] : 0.f;
                }
                zs[__brev((unsigned)m) >> (32 - logM)] = make_float2(v0, v1);
            }
        }
        fft_lds_sub(zs, pl.twiddle, M, logM, 1, tid, 256);
        if (live) {
            for (int k = tid; k < bins; k += 256) {
                const float2 zk = zs[k & (M - 1)], zm = zs[(M - k) & (M - 1)];
                const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
                const float2 b = make_float2(0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y));
                const float2 w = k < M ? pl.twiddle[k] : make_float2(-1.f, 0.f);
                const float2 wb = cmul(w, b);                              // X = E - i * w * B
                if constexpr (kPseudo) {
                    const float2 xv = make_float2(e.x + wb.y, e.y - wb.x);
                    tile[k * F + f] = pass == 1 ? sub_rounded(xv, tile[k * F + f]) : xv;
                } else {
                    tile[k * F + f] = make_float2(e.x + wb.y, e.y - wb.x);
                }
            }
        }
        __syncthreads();
    }
    if constexpr (kRows || kCrops<SRC>) {            // [T][2][bins]: a frame's bins lie together, so consecutive lanes run along k
        // (the tile is [bins][F], so these LDS reads stride F values and conflict on banks; lanes along f would read it conflict-free
        // and scatter the global stores over F rows instead.  Coalesced stores were preferred: profiles/pitch.md has the kernel's share)
        for (int idx = threadIdx.x; idx < bins * nf; idx += 1024) {
            const int f = idx / bins, k = idx - f * bins;
            spec[((long long)(t0 + f) * 2 + ch) * bins + k] = tile[k * F + f];
        }
    } else for (int idx = threadIdx.x; idx < bins * F; idx += 1024) {
        const int k = idx / F, f = idx - k * F;
        if constexpr (kStream<SRC>) {
            if (f < nf) ss.ring[((long long)ch * bins + k) * ss.R + (t0 + f) % ss.R] = tile[idx];
        } else if constexpr (kGrad) {
            if (f < nf) {
                const long long e = ((long long)ch * bins + k) * T + t0 + f;
                const bool edge = k == 0 || k == M;                 // irfft reads neither imaginary part: c_k = 1, no gradient there
                const float c = (edge ? 1.f : 2.f) / (float)n;
                float2 gv = tile[idx];
                gv = make_float2(gv.x * c, edge ? 0.f : gv.y * c);
                const float2 xv = gd.X[e];
                if (gd.l1_scale != 0.f) {                           // + sgn(|p| - |y|) p / |p| / n_el, p = mask X; 0 where |p| = 0 or |p| = |y|
                    const float2 p = cmul(gd.mask[e], xv), yv = gd.Y[e];
                    const float ap = hypotf(p.x, p.y), ay = hypotf(yv.x, yv.y);
                    if (ap > 0.f && ap != ay) {
                        const float s = (ap > ay ? gd.l1_scale : -gd.l1_scale) / ap;
                        gv.x = fmaf(s, p.x, gv.x); gv.y = fmaf(s, p.y, gv.y);
                    }
                }
                gd.dmask[e] = make_float2(gv.x * xv.x + gv.y * xv.y, gv.y * xv.x - gv.x * xv.y);        // times conj(X)
            }
        } else if constexpr (kPseudo) {
            if (f < nf) (pass == 0 ? ps.inst : spec)[((long long)ch * bins + k) * T + t0 + f] = tile[idx];
        } else {
            if (f < nf) spec[((long long)ch * bins + k) * T + t0 + f] = tile[idx];
        }
    }
    if constexpr (kPseudo) {
        if (pass == 0) {
            pass = 1;
            in.wv = mix_wv;
            __syncthreads();                         // the Y tile is read out before pass 1 writes D over it
            goto second_pass;
        }
    }
    if constexpr (kStream<SRC>) {                    // the samples the next step's first frames reach back to
        if (blockIdx.x == 0) {
            const int keep = (int)(ss.L - ss.tail_out_base);
            for (int i = threadIdx.x; i < keep; i += 1024) {
                if constexpr (kPcm) ss.tail_out[(long long)ch * ss.tail_pitch + i] = stream_sample_pcm(ss, in, ch, ss.tail_out_base + i);
                else ss.tail_out[(long long)ch * ss.tail_pitch + i] = stream_sample(ss, ch, ss.tail_out_base + i);
            }
        }
    }
}

// The final mask at (row, t): mask_a, or the TTA average with mask_b shifted by `shift`, then the merge_artifacts blend wgt[t].
__device__ __forceinline__ float2 final_mask(const float2* __restrict__ ma, int Wa, const float2* __restrict__ mb, int Wb, int shift,
                                             const float* __restrict__ wgt, long long row, int t) {
    float2 m = ma[row * Wa + t];
    if (mb) {
        const float2 b = mb[row * Wb + t + shift];
        m = make_float2((m.x + b.x) * 0.5f, (m.y + b.y) * 0.5f);
    }
    if (wgt) {        // inference.py:27-30: |m| through merge_artifacts, the phase kept (np.angle(0) = 0: m' = w where m = 0)
        const float mag = hypotf(m.x, m.y), w = wgt[t];
        const float nm = mag + w * (1.f - mag);
        m = mag > 0.f ? make_float2(nm * (m.x / mag), nm * (m.y / mag)) : make_float2(nm, 0.f);
    }
    return m;
}

// (evaluation form) what the workgroup keeps of its song, and a thread's share of a segment's sums; empty in every other form, so
// that those keep their code as it was
struct EvalSong { WaveEval e; const float* mix; long long L; };         // the song's entry, its mixture [2][L]
struct EvalSeg { double q[4]; long long bound; };                       // reference and error squares of the lower, then of the upper window
struct EvalNone {};
template <bool EVAL> using EvalLocal = typename std::conditional<EVAL, EvalSong, EvalNone>::type;
template <bool EVAL> using EvalSums = typename std::conditional<EVAL, EvalSeg, EvalNone>::type;
struct WindowSums {};                                                   // behind const WaveEval* in the pack: the evaluation's second launch
template <class X, class... T> constexpr bool kHasType = (std::is_same<X, T>::value || ...);

// The second launch of an evaluation, blockIdx = (window, song), 256 threads: one wave (64 lanes) per quantity q = 2 * stem + (0: reference
// square, 1: error square).  The window's items are (segment, channel, wave of the segment's group), in that order; lane l adds items l,
// l + 64, ... and the xor butterfly adds the lanes: a fixed order, so two calls give the same bits.  The window's first segment may begin in
// the window before: its upper slots are taken.
__device__ __forceinline__ void eval_window_sums(int M, const SongSeg& sg, const WaveEval& ev) {
    const long long samples = (long long)M * (sg.T - 1), lo = (long long)blockIdx.x * ev.window;
    if (lo >= samples) return;
    const long long hi = lo + ev.window < samples ? lo + ev.window : samples;
    const long long s0 = lo / M, s1 = (hi - 1) / M, items = (s1 - s0 + 1) * 8;
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63, stem = q >> 1, k = q & 1;
    double acc = 0.0;
    for (long long it = lane; it < items; it += 64) {
        const long long s = s0 + (it >> 3);
        const int ch = (int)(it >> 2) & 1, wv = (int)it & 3;
        const int slot = s * M >= lo ? 0 : 2;
        acc += ev.part[((((long long)stem * 2 + ch) * (sg.T - 1) + s) * 4 + wv) * 4 + slot + k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) ev.sums[(long long)blockIdx.x * 4 + q] = acc;
}

// which: 0 = plain spectrogram (mask_a null) / instruments y = m X, 1 = vocals v = (1 - m) X
// CPLX: the mask is complex64 (is_complex handles), y = m X and v = (1 - m) X as complex products
// OUT (at most one type): where the samples go -- none = WaveF32Out (planar float32, as documented); WavePcm16Out: `wave` / the table's
// y_wave, v_wave then point to interleaved int16 [samples][2] (streams: [capacity][2], segment s at sample (s - t_out) * M); the carry
// and `prev` stay float.  const WaveEval* (SRC = const SongSeg only): the evaluation form -- one WaveEval per song beside
// the song table, behind the kernel's `wave` pointer (which the table forms do not read).  Where the plain form stores sample p of channel
// ch, this form takes the same float, the true stem's sample from the song's `inst` wave (which 1: the table's mixture minus it, formed in
// double) and adds the reference square and the error square, in double, to the segment's lower or upper window (window >= hop: a segment
// of hop samples meets at most two).  A segment belongs to one group of 256 threads, so its sums are reduced by wave shuffles alone and
// lane 0 of each of the group's four waves writes that wave's four partials.  With WindowSums behind it in the pack the kernel is the
// evaluation's second launch instead (eval_window_sums above: grid (window, song), 256 threads, no LDS), which adds them per window in a
// fixed order -- under this kernel's name, like every form of this file, so that the launch profiler's report keeps one name per stage.
template <bool CPLX, class SRC = const float2, class... OUT>
__global__ __launch_bounds__(1024) void istft_tile_kernel(FFTPlan pl, SRC* __restrict__ src, int T, int S,
                                                          const float* __restrict__ ma, int Wa, const float* __restrict__ mb, int Wb,
                                                          int shift, const float* __restrict__ wgt, int which,
                                                          float* __restrict__ wave, long long out_len) {
    constexpr bool kSums = kHasType<WindowSums, OUT...>;
    static_assert(sizeof...(OUT) <= (kSums ? 2 : 1), "one destination type at most");
    constexpr bool kEval = std::is_same<typename FirstOr<void, OUT...>::type, const WaveEval*>::value;
    static_assert((!kEval || kSongTable<SRC>) && (!kSums || kEval), "the evaluation forms are song-table forms");
    if constexpr (kSums) {
        eval_window_sums(pl.n_fft >> 1, src[blockIdx.y], reinterpret_cast<const WaveEval*>(wave)[blockIdx.y]);
        return;
    }
    using DST = typename std::conditional<kEval, WaveF32Out, typename FirstOr<WaveF32Out, OUT...>::type>::type;
    extern __shared__ __attribute__((aligned(16))) float2 lds2[];
    const int n = pl.n_fft, M = n >> 1, bins = M + 1, logM = pl.log2n - 1, F = S + 1;
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    float2* zs = lds2 + (size_t)g * M;                              // this group's FFT buffer = its time-domain frame afterwards
    float2* tile = lds2 + (size_t)TG * M;                           // [bins][F]
    float* prev = reinterpret_cast<float*>(tile + (size_t)bins * F);   // [M] windowed second half of the last frame of the previous round
    int t0 = blockIdx.x * S;
    const int ch = blockIdx.y;
    const float2* __restrict__ spec;
    StreamLocal<SRC> ss{};
    PairLocal<SRC> pr{};
    TripleLocal<SRC> tr{};
    EvalLocal<kEval> ev{};
    bool carried = false;                           // (stream) frame t0 of this workgroup comes from the carry, not from the ring
    if constexpr (kStream<SRC>) {                    // blockIdx.z = table entry; the frames [t_out, t_done) of its stream, from its rings
        ss = src[blockIdx.z];
        if (t0 >= ss.t_done - 1 - ss.t_out) return;                 // (an entry with nothing turning final has no segment at all)
        t0 += ss.t_out; T = ss.t_done;
        spec = ss.ring; ma = ss.mask_a; mb = ss.mask_b; shift = ss.shift;
        wave = which ? ss.v_wave : ss.y_wave;
        carried = ss.carried && blockIdx.x == 0;
    } else if constexpr (kSongTable<SRC>) {          // blockIdx.z = song; writes that song's y_wave (which 0) or v_wave (which 1)
        const SongSeg sg = src[blockIdx.z];
        if (t0 >= sg.T - 1) return;
        spec = sg.spec; T = sg.T;
        ma += (long long)(CPLX ? 2 : 1) * sg.mcol_a;
        if (mb) mb += (long long)(CPLX ? 2 : 1) * sg.mcol_b;
        if (wgt) wgt += sg.frame0;
        if constexpr (kEval) { ev.e = reinterpret_cast<const WaveEval*>(wave)[blockIdx.z]; ev.mix = sg.wave; ev.L = sg.L; }
        wave = which ? sg.v_wave : sg.y_wave;
        out_len = (long long)M * (sg.T - 1);
    } else if constexpr (kPair<SRC>) {
        pr = src[0];
        spec = nullptr;
    } else if constexpr (kTriple<SRC>) {
        tr = src[0];
        spec = nullptr;
    } else {
        spec = src;
    }
    const int nf = (T - t0) < F ? (T - t0) : F;
    float s_yp = 0.f, s_yy = 0.f, s_pp = 0.f;        // (pair, triple) this thread's share of <y, p>, <y, y>, <p, p>
    float s_nq = 0.f, s_nn = 0.f, s_qq = 0.f;        // (triple) ... and of <n, q>, <n, n>, <q, q>, n = x - y and q = x - p sample by sample
    // (pair) pass 0 = the target y, pass 1 = the estimate p; a thread handles the same samples in both, so pass 1 reads back its own stores
    // (triple) pass 0 = the mixture x, 1 = y, 2 = p: pass 1 reads back its own x store, pass 2 its own x and y stores
    for (int pass = 0; pass < (kTriple<SRC> ? 3 : kPair<SRC> ? 2 : 1); ++pass) {
        for (int idx = threadIdx.x; idx < bins * F; idx += 1024) {
            const int k = idx / F, f = idx - k * F;
            float2 v = make_float2(0.f, 0.f);
            if constexpr (kPair<SRC>) {
                if (f < nf) {
                    const long long row = (long long)ch * bins + k;
                    const int t = t0 + f;
                    if (pass == 0) {
                        v = pr.y[row * pr.y_pitch + pr.y_off + t];
                    } else {
                        v = pr.x[row * pr.x_pitch + t];
                        if (pr.mask) v = cmul(pr.mask[row * pr.x_pitch + t], v);
                    }
                }
            } else if constexpr (kTriple<SRC>) {
                if (f < nf) {
                    const long long row = (long long)ch * bins + k;
                    const int t = t0 + f;
                    const long long e = row * tr.xy_pitch + tr.xy_off + t;
                    if (pass == 0) v = tr.x[e];
                    else if (pass == 1) v = tr.y[e];
                    else if (tr.mask) v = cmul(tr.mask[e], tr.x[e]);
                    else v = tr.p[row * tr.p_pitch + t];
                }
            } else if constexpr (kStream<SRC>) {
                if (f < nf && !(carried && f == 0)) {
                    const long long row = (long long)ch * bins + k;
                    const int t = t0 + f;
                    v = spec[row * ss.R + t % ss.R];
                    const long long ca = row * ss.RM + t % ss.RM, cb = row * ss.RM + (t + shift) % ss.RM;
                    if constexpr (CPLX) {
                        float2 m = reinterpret_cast<const float2*>(ma)[ca];
                        if (mb) {
                            const float2 b = reinterpret_cast<const float2*>(mb)[cb];
                            m = make_float2((m.x + b.x) * 0.5f, (m.y + b.y) * 0.5f);
                        }
                        if (ss.fmin_ring) {             // (--postprocess stream: final_mask's blend, the weight from the stream's ring)
                            const float mag = hypotf(m.x, m.y), w = ss.wgt_ring[t % ss.RW];
                            const float nm = mag + w * (1.f - mag);
                            m = mag > 0.f ? make_float2(nm * (m.x / mag), nm * (m.y / mag)) : make_float2(nm, 0.f);
                        }
                        const float2 gm = which ? make_float2(1.f - m.x, -m.y) : m;
                        v = cmul(gm, v);
                    } else {
                        float m = ma[ca];
                        if (mb) m = (m + mb[cb]) * 0.5f;
                        if (ss.fmin_ring) m += ss.wgt_ring[t % ss.RW] * (1.f - m);
                        const float gm = which ? 1.f - m : m;
                        v = make_float2(gm * v.x, gm * v.y);
                    }
                }
            } else if (f < nf) {
                const long long row = (long long)ch * bins + k;
                const int t = t0 + f;
                v = spec[row * T + t];
                if constexpr (CPLX) {
                    if (ma) {
                        const float2 m = final_mask(reinterpret_cast<const float2*>(ma), Wa, reinterpret_cast<const float2*>(mb), Wb, shift,
                                                    wgt, row, t);
                        const float2 gm = which ? make_float2(1.f - m.x, -m.y) : m;
                        v = cmul(gm, v);
                    }
                } else if (ma) {
                    float m = ma[row * Wa + t];
                    if (mb) m = (m + mb[row * Wb + t + shift]) * 0.5f;
                    if (wgt) m += wgt[t] * (1.f - m);
                    const float gm = which ? 1.f - m : m;                // y = m X, v = (1 - m) X  (inference.py:32-38; same form as apply_mask)
                    v = make_float2(gm * v.x, gm * v.y);
                }
            }
            tile[idx] = v;
        }
        __syncthreads();
        const float invM = 1.f / (float)M;
        for (int f0 = 0; f0 < nf; f0 += TG) {
            const int f = f0 + g;
            const bool live = f < nf;
            if (live) {
                // Z[k] = E[k] + i O[k];  loaded as conj(Z) so that a forward FFT gives conj(M * z)
                for (int k = tid; k < M; k += 256) {
                    float2 xk = tile[k * F + f], xm = tile[(M - k) * F + f];
                    if (k == 0) { xk.y = 0.f; xm.y = 0.f; }             // numpy's irfft ignores the imaginary parts of DC and Nyquist
                    const float2 e = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
                    const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
                    const float2 w = pl.twiddle[k];                     // e^{-2 pi i k / N}; O = conj(w) * d
                    const float2 o = make_float2(w.x * d.x + w.y * d.y, w.x * d.y - w.y * d.x);
                    const float2 z = make_float2(e.x - o.y, e.y + o.x); // E + i O
                    zs[__brev((unsigned)k) >> (32 - logM)] = make_float2(z.x, -z.y);
                }
            }
            fft_lds_sub(zs, pl.twiddle, M, logM, 1, tid, 256);
            // in place: zs[m] = (x[2m], x[2m+1]) windowed -> the group's buffer is the windowed frame, as floats [n_fft]
            if (live) {
                bool from_carry = false;
                if constexpr (kStream<SRC>) from_carry = carried && f == 0;
                if (from_carry) {                        // only the windowed second half of that frame is used: floats [M, 2M) of the buffer
                    if constexpr (kStream<SRC>) {
                        const float* cin = ss.carry_in + (long long)(which * 2 + ch) * M;
                        for (int m = tid; m < M; m += 256)
                            zs[m] = 2 * m >= M ? make_float2(cin[2 * m - M], cin[2 * m + 1 - M]) : make_float2(0.f, 0.f);
                    }
                } else {
                    for (int m = tid; m < M; m += 256) {
                        const float2 r = zs[m];
                        zs[m] = make_float2(r.x * invM * pl.window[2 * m], -r.y * invM * pl.window[2 * m + 1]);
                    }
                }
            }
            __syncthreads();
            // segment s = t - 1 = second half of frame t-1 (previous group's buffer, or `prev` for group 0) + first half of frame t
            if (live && f > 0) {
                const int s = t0 + f - 1;
                const float* cur = reinterpret_cast<const float*>(zs);
                const float* before = g == 0 ? prev : reinterpret_cast<const float*>(zs - M) + M;
                // (evaluation) `bound` = the first sample of the segment's upper window (the quotient in double: exact below 2^53, then
                // corrected by one)
                EvalSums<kEval> es{};
                if constexpr (kEval) {
                    const long long p0 = (long long)s * M;
                    long long w = (long long)((double)p0 / (double)ev.e.window);
                    if (w * ev.e.window > p0) --w;
                    else if ((w + 1) * ev.e.window <= p0) ++w;
                    es.bound = (w + 1) * ev.e.window;
                }
                for (int i = tid; i < M; i += 256) {
                    const float w0 = pl.window[i], w2 = pl.window[i + M];
                    const float ws = fmaf(w0, w0, w2 * w2);
                    const float a = before[i] + cur[i];
                    if constexpr (kPair<SRC>) {                       // (s <= T - 2: every sample lies inside [0, hop (T-1)))
                        const long long p = (long long)ch * out_len + (long long)s * M + i;
                        const float v = ws > FLT_MIN ? a / ws : a;
                        if (pass == 0) {
                            pr.y_wave[p] = v;
                            s_yy = fmaf(v, v, s_yy);
                        } else {
                            pr.p_wave[p] = v;
                            s_yp = fmaf(pr.y_wave[p], v, s_yp);
                            s_pp = fmaf(v, v, s_pp);
                        }
                    } else if constexpr (kTriple<SRC>) {              // (s <= T - 2, as above)
                        const long long p = (long long)ch * out_len + (long long)s * M + i;
                        const float v = ws > FLT_MIN ? a / ws : a;
                        if (pass == 0) {
                            tr.x_wave[p] = v;
                        } else if (pass == 1) {
                            const float nv = tr.x_wave[p] - v;
                            tr.y_wave[p] = v;
                            s_yy = fmaf(v, v, s_yy);
                            s_nn = fmaf(nv, nv, s_nn);
                        } else {
                            const float xv = tr.x_wave[p], yv = tr.y_wave[p];
                            const float nv = xv - yv, qv = xv - v;
                            tr.p_wave[p] = v;
                            s_yp = fmaf(yv, v, s_yp);
                            s_pp = fmaf(v, v, s_pp);
                            s_nq = fmaf(nv, qv, s_nq);
                            s_qq = fmaf(qv, qv, s_qq);
                        }
                    } else if constexpr (kStream<SRC>) {
                        // (the float store written out: through put() hipcc allocates this instantiation's registers differently)
                        if constexpr (DST::kInterleaved) DST::put(wave, 0, ch, (long long)(s - ss.t_out) * M, i, ws > FLT_MIN ? a / ws : a);
                        else wave[(long long)ch * ss.out_pitch + (long long)(s - ss.t_out) * M + i] = ws > FLT_MIN ? a / ws : a;
                    } else if constexpr (kEval) {                     // (s <= T - 2: every sample lies inside [0, hop (T-1)), and hop (T-1) <= L)
                        const long long p = (long long)s * M + i;
                        const float v = ws > FLT_MIN ? a / ws : a;
                        if (ev.e.store) wave[(long long)ch * out_len + p] = v;
                        double r = (double)ev.e.inst[(long long)ch * ev.L + p];
                        if (which) r = (double)ev.mix[(long long)ch * ev.L + p] - r;
                        const double d = r - (double)v;
                        if (p < es.bound) { es.q[0] = fma(r, r, es.q[0]); es.q[1] = fma(d, d, es.q[1]); }
                        else { es.q[2] = fma(r, r, es.q[2]); es.q[3] = fma(d, d, es.q[3]); }
                    } else {
                        const long long p = (long long)s * M + i;
                        if (p < out_len) DST::put(wave, out_len, ch, p, 0, ws > FLT_MIN ? a / ws : a);
                    }
                }
                if constexpr (kEval) {                               // the wave's four sums by the xor butterfly: the same order every time
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) es.q[j] += __shfl_xor(es.q[j], off, 64);
                    }
                    if ((tid & 63) == 0) {
                        double* dst = ev.e.part + ((((long long)which * 2 + ch) * (T - 1) + s) * 4 + (tid >> 6)) * 4;
#pragma unroll
                        for (int j = 0; j < 4; ++j) dst[j] = es.q[j];
                    }
                }
            }
            __syncthreads();
            // carry: the last live frame of this round leaves its second half for the next round's group 0
            {
                const int last = (nf - f0 < TG ? nf - f0 : TG) - 1;
                if (g == last) {
                    const float* cur = reinterpret_cast<const float*>(zs);
                    for (int i = tid; i < M; i += 256) prev[i] = cur[M + i];
                }
            }
            __syncthreads();
        }
    }
    if constexpr (kPair<SRC>) {                      // the workgroup's three sums, in a fixed order: wave, then the 16 waves by index
        float* red = reinterpret_cast<float*>(tile);                // (the tile is dead: the last round ended with a barrier)
        float v3[3] = {s_yp, s_yy, s_pp};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v3[j] += __shfl_xor(v3[j], off, 64);
            if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 3 + j] = v3[j];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            float s = 0.f;
            for (int w = 0; w < 16; ++w) s += red[w * 3 + threadIdx.x];
            pr.part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = s;
        }
    }
    if constexpr (kTriple<SRC>) {                    // the workgroup's six sums, in the same fixed order
        float* red = reinterpret_cast<float*>(tile);
        float v6[6] = {s_yp, s_yy, s_pp, s_nq, s_nn, s_qq};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v6[j] += __shfl_xor(v6[j], off, 64);
            if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 6 + j] = v6[j];
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            float s = 0.f;
            for (int w = 0; w < 16; ++w) s += red[w * 6 + threadIdx.x];
            tr.part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = s;
        }
    }
    if constexpr (kStream<SRC>) {                    // the workgroup that ends the step hands its last half frame to the next step
        if (t0 + nf == ss.t_done) {
            float* cout = ss.carry_out + (long long)(which * 2 + ch) * M;
            for (int i = threadIdx.x; i < M; i += 1024) cout[i] = prev[i];
        }
    }
}

static int tile_frames(const FFTPlan& pl, int extra_floats) {
    // largest F <= 17 with TG FFT buffers + tile[bins][F] (+ extra) inside 150 KB of LDS
    const int M = pl.n_fft / 2, bins = M + 1;
    long long budget = 150 * 1024 - (long long)TG * M * 8 - (long long)extra_floats * 4;
    int F = (int)(budget / ((long long)bins * 8));
    return F > 17 ? 17 : F;
}

static bool tiled_signal_path(const FFTPlan& pl, int hop) {
    static const bool on = !getenv("VR_NO_TILED_STFT");
    return on && hop * 2 == pl.n_fft && pl.n_fft >= 128 && tile_frames(pl, pl.n_fft / 2) >= 3;
}

template <bool CPLX, class... OUT>
static void launch_istft_tile(const FFTPlan& pl, const float2* spec, int hop, int T, const float* mask_a, int Wa, const float* mask_b,
                              int Wb, int shift, const float* wgt, int which, float* wave, hipStream_t st) {
    const int M = pl.n_fft / 2, bins = M + 1;
    const long long out_len = (long long)hop * (T - 1);
    if (out_len <= 0) return;
    const int F = tile_frames(pl, M);
    const int S = F - 1;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8 + (size_t)M * 4;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<CPLX, const float2, OUT...>), 160 * 1024);
    // per stem: the complex spectrogram (8 B per bin-frame), the mask(s) (4 B, complex 8 B), hop samples written per frame, two channels
    prof_note(0.0, 2.0 * ((double)bins * T * (8.0 + (CPLX ? 8.0 : 4.0) * (mask_b ? 2 : 1)) + (sizeof...(OUT) ? 2.0 : 4.0) * (double)out_len));
    VR_LAUNCH((istft_tile_kernel<CPLX, const float2, OUT...>), dim3((unsigned)((T - 1 + S - 1) / S), 2), dim3(1024), lds, st, pl, spec, T, S, mask_a, Wa,
              mask_b, Wb, shift, wgt, which, wave, out_len);
    VR_HIP(hipGetLastError());
}

void launch_istft_masked(const FFTPlan& pl, const float2* spec, int hop, int T, const float* mask_a, int Wa, const float* mask_b,
                         int Wb, int shift, const float* wgt, int which, float* wave, hipStream_t st) {
    launch_istft_tile<false>(pl, spec, hop, T, mask_a, Wa, mask_b, Wb, shift, wgt, which, wave, st);
}

void launch_istft_masked_pcm16(const FFTPlan& pl, const float2* spec, int hop, int T, bool cplx, const float* mask_a, int Wa,
                               const float* mask_b, int Wb, int shift, const float* wgt, int which, int16_t* out, hipStream_t st) {
    float* w = reinterpret_cast<float*>(out);
    if (cplx) launch_istft_tile<true, WavePcm16Out>(pl, spec, hop, T, mask_a, Wa, mask_b, Wb, shift, wgt, which, w, st);
    else launch_istft_tile<false, WavePcm16Out>(pl, spec, hop, T, mask_a, Wa, mask_b, Wb, shift, wgt, which, w, st);
}

void launch_istft_masked_complex(const FFTPlan& pl, const float2* spec, int hop, int T, const float2* mask_a, int Wa,
                                 const float2* mask_b, int Wb, int shift, const float* wgt, int which, float* wave, hipStream_t st) {
    launch_istft_tile<true>(pl, spec, hop, T, reinterpret_cast<const float*>(mask_a), Wa, reinterpret_cast<const float*>(mask_b), Wb,
                            shift, wgt, which, wave, st);
}

bool wave_loss_available(const FFTPlan& pl, int hop) { return tiled_signal_path(pl, hop); }

int wave_pair_blocks(const FFTPlan& pl, int T) {
    const int S = tile_frames(pl, pl.n_fft / 2) - 1;
    return T < 2 ? 0 : (T - 1 + S - 1) / S;
}

// The pair and the triple form of istft_tile_kernel: one body, the table entry's type picks the kernel instance
template <class TABLE>
static void launch_istft_table(const FFTPlan& pl, const TABLE* table_dev, const TABLE& t, int signals, int T, hipStream_t st) {
    constexpr bool kTriple = std::is_same<TABLE, WaveTriple>::value;
    const int M = pl.n_fft / 2, bins = M + 1;
    const int nb = wave_pair_blocks(pl, T);
    if (nb == 0) return;
    if constexpr (kTriple)
        VR_CHECK(t.xy_off >= 0 && t.xy_off + T <= t.xy_pitch && (t.mask || (t.p && T <= t.p_pitch)) && signals > 0, -2,
                 "triple iSTFT: the frames leave their rows");
    else
        VR_CHECK(t.y_off >= 0 && t.y_off + T <= t.y_pitch && T <= t.x_pitch && signals > 0, -2, "pair iSTFT: the frames leave their rows");
    const int F = tile_frames(pl, M);
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8 + (size_t)M * 4;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<true, const TABLE>), 160 * 1024);
    // every spectrogram read once (pair: target and estimate; triple: the mixture too; fused: the mask and the mixture again), the waves
    // written, the target's wave (triple: the mixture's twice as well) read back by the thread that stored it
    prof_note(0.0, (double)signals * ((double)bins * T * 8.0 * ((kTriple ? 3 : 2) + (t.mask ? 1 : 0)) + (kTriple ? 6.0 : 3.0) * 4.0 * (double)M * (T - 1)));
    if constexpr (kTriple)
        VR_LAUNCH((istft_tile_kernel<true, const WaveTriple>), dim3((unsigned)nb, (unsigned)signals), dim3(1024), lds, st, pl, table_dev, T, F - 1,
                  (const float*)nullptr, 0, (const float*)nullptr, 0, 0, (const float*)nullptr, 0, (float*)nullptr, (long long)M * (T - 1));
    else
        VR_LAUNCH((istft_tile_kernel<true, const WavePair>), dim3((unsigned)nb, (unsigned)signals), dim3(1024), lds, st, pl, table_dev, T, F - 1,
                  (const float*)nullptr, 0, (const float*)nullptr, 0, 0, (const float*)nullptr, 0, (float*)nullptr, (long long)M * (T - 1));
    VR_HIP(hipGetLastError());
}

void launch_istft_pair(const FFTPlan& pl, const WavePair* pair_dev, const WavePair& pair, int signals, int T, hipStream_t st) {
    launch_istft_table(pl, pair_dev, pair, signals, T, st);
}

void launch_istft_triple(const FFTPlan& pl, const WaveTriple* triple_dev, const WaveTriple& tr, int signals, int T, hipStream_t st) {
    launch_istft_table(pl, triple_dev, tr, signals, T, st);
}

// the table entry on its way to the device: through the caller's staging slot on the stream, or (no slot) synchronously
template <class TABLE>
static const TABLE* send_wave_table(const TABLE& t, float* table_dev, WaveTable* staging, hipStream_t st) {
    if (staging) {
        memcpy(staging, &t, sizeof(TABLE));
        VR_HIP(hipMemcpyAsync(table_dev, staging, sizeof(TABLE), hipMemcpyHostToDevice, st));
    } else {
        VR_HIP(hipMemcpy(table_dev, &t, sizeof(TABLE), hipMemcpyHostToDevice));
    }
    return reinterpret_cast<const TABLE*>(table_dev);
}

void launch_wave_term(const FFTPlan& pl, const WavePair& pair, float* table_dev, WaveTable* staging, int signals, int T, float* sums,
                      hipStream_t st) {
    launch_istft_pair(pl, send_wave_table(pair, table_dev, staging, st), pair, signals, T, st);
    launch_reduce_rows(pair.part, 3, signals * wave_pair_blocks(pl, T), sums, 3, 0, 1.f, st);
}

void launch_wave_term(const FFTPlan& pl, const WaveTriple& tr, float* table_dev, WaveTable* staging, int signals, int T, float* sums,
                      hipStream_t st) {
    launch_istft_triple(pl, send_wave_table(tr, table_dev, staging, st), tr, signals, T, st);
    launch_reduce_rows(tr.part, 6, signals * wave_pair_blocks(pl, T), sums, 6, 0, 1.f, st);
}

WaveTermFloats wave_term_floats(const FFTPlan& pl, int hop, int kind, int signals, int T) {
    const int waves = kind == 3 ? 3 : 2;
    return WaveTermFloats{waves, (size_t)signals * hop * (T - 1), (size_t)signals * wave_pair_blocks(pl, T) * (waves == 3 ? 6 : 3), 64};
}

// The two- and the three-wave gradient form of stft_tile_kernel: one body, the argument struct's type picks the kernel instance
template <class GRAD>
static void launch_wave_grad(const FFTPlan& pl, const GRAD& g, int signals, int T, hipStream_t st) {
    constexpr bool kThree = std::is_same<GRAD, WaveGrad3>::value;
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const float, GRAD>), 160 * 1024);
    // two or three waves read, X (and mask, Y with the L1 part) read, dmask written
    prof_note(0.0, (double)signals * ((kThree ? 3.0 : 2.0) * 4.0 * (double)M * (T - 1) + 8.0 * (double)bins * T * (g.l1_scale != 0.f ? 4 : 2)));
    if constexpr (kThree)
        VR_LAUNCH((stft_tile_kernel<const float, WaveGrad3>), dim3((unsigned)((T + F - 1) / F), (unsigned)signals), dim3(1024), lds, st, pl,
                  (const float*)nullptr, (long long)M * (T - 1), T, F, (float2*)nullptr, g);
    else
        VR_LAUNCH((stft_tile_kernel<const float, WaveGrad>), dim3((unsigned)((T + F - 1) / F), (unsigned)signals), dim3(1024), lds, st, pl,
                  (const float*)nullptr, (long long)M * (T - 1), T, F, (float2*)nullptr, g);
    VR_HIP(hipGetLastError());
}

void launch_stft_wave_grad3(const FFTPlan& pl, const WaveGrad3& g, int signals, int T, hipStream_t st) { launch_wave_grad(pl, g, signals, T, st); }

void launch_stft_wave_grad(const FFTPlan& pl, const WaveGrad& g, int signals, int T, hipStream_t st) { launch_wave_grad(pl, g, signals, T, st); }

// irfft(spec[:, t]) * window -> frames[ch][t][0..n)
__global__ __launch_bounds__(256) void istft_frame_kernel(FFTPlan pl, const float2* __restrict__ spec, int T,
                                                          float* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) float2 xs[];
    const int n = pl.n_fft, t = blockIdx.x, ch = blockIdx.y;
    const int bins = n / 2 + 1;
    const float2* sp = spec + (long long)ch * bins * T + t;
    // inverse via forward FFT of the conjugate spectrum (Hermitian-extended); imaginary parts of
    // the DC and Nyquist bins are ignored like numpy's irfft does.
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        float2 v;
        if (k < bins) {
            v = sp[(long long)k * T];
            v.y = -v.y;
            if (k == 0 || k == n / 2) v.y = 0.f;
        } else {
            v = sp[(long long)(n - k) * T];      // conj(conj(X[n-k])) = X[n-k]
        }
        const int r = __brev((unsigned)k) >> (32 - pl.log2n);
        xs[r] = v;
    }
    fft_lds(xs, pl.twiddle, n, pl.log2n);
    const float inv = 1.f / (float)n;
    float* fr = frames + ((long long)ch * T + t) * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) fr[i] = xs[i].x * inv * pl.window[i];
}

__global__ void istft_ola_kernel(FFTPlan pl, const float* __restrict__ frames, int hop, int T, long long out_len,
                                 float* __restrict__ wave) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = blockIdx.y;
    if (p >= out_len) return;
    const int n = pl.n_fft;
    const long long q = p + n / 2;
    long long t_hi = q / hop;
    if (t_hi > T - 1) t_hi = T - 1;
    long long t_lo = (q - n + hop) / hop;          // smallest t with t*hop + n > q
    if (q - n + 1 <= 0) t_lo = 0;
    if (t_lo < 0) t_lo = 0;
    float acc = 0.f, wss = 0.f;
    for (long long t = t_lo; t <= t_hi; ++t) {
        const int i = (int)(q - t * hop);
        if (i < 0 || i >= n) continue;
        acc += frames[((long long)ch * T + t) * n + i];
        const float w = pl.window[i];
        wss = fmaf(w, w, wss);
    }
    wave[(long long)ch * out_len + p] = (wss > FLT_MIN) ? acc / wss : acc;
}

void launch_stft_tiled(const FFTPlan& pl, const float* wave, long long L, int T, float2* spec, hipStream_t st) {
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;                                     // whole rounds of TG frames
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<>), 160 * 1024);
    prof_note(0.0, 2.0 * (4.0 * (double)L + 8.0 * (double)bins * T));              // unique audio read once, complex64 spectrogram written
    VR_LAUNCH((stft_tile_kernel<>), dim3((unsigned)((T + F - 1) / F), 2), dim3(1024), lds, st, pl, wave, L, T, F, spec);
    VR_HIP(hipGetLastError());
}

void launch_stft_pcm(const FFTPlan& pl, const PcmIn& in, long long L, int T, float2* spec, hipStream_t st) {
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const float, PcmIn>), 160 * 1024);
    prof_note(0.0, (double)pcm_sample_bytes(in.fmt) * in.channels * (double)L + 2.0 * 8.0 * (double)bins * T);
    VR_LAUNCH((stft_tile_kernel<const float, PcmIn>), dim3((unsigned)((T + F - 1) / F), 2), dim3(1024), lds, st, pl, (const float*)nullptr, L, T, F,
              spec, in);
    VR_HIP(hipGetLastError());
}

void launch_stft_rows(const FFTPlan& pl, const float* wave, long long L, int T, float2* rows, hipStream_t st) {
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const float, SpecRows>), 160 * 1024);
    prof_note(0.0, 2.0 * (4.0 * (double)L + 8.0 * (double)bins * T));
    VR_LAUNCH((stft_tile_kernel<const float, SpecRows>), dim3((unsigned)((T + F - 1) / F), 2), dim3(1024), lds, st, pl, wave, L, T, F, rows,
              SpecRows{});
    VR_HIP(hipGetLastError());
}

bool stft_crops_supported(int n_fft, int hop) {
    if (n_fft <= 0 || (n_fft & (n_fft - 1))) return false;
    return tiled_signal_path(FFTPlan{n_fft, 0, nullptr, nullptr}, hop);
}

// rows_total: the rows the call writes, both channels of every entry counted once (the profiler's byte note)
void launch_stft_crops(const FFTPlan& pl, const CropSeg* table_dev, int entries, int max_T, double rows_total, hipStream_t st) {
    if (entries <= 0 || max_T <= 0) return;
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const CropSeg>), 160 * 1024);
    prof_note(0.0, rows_total * 2.0 * (4.0 * (double)M + 8.0 * (double)bins));      // a row reads one hop of new samples a channel
    VR_LAUNCH((stft_tile_kernel<const CropSeg>), dim3((unsigned)((max_T + F - 1) / F), 2, (unsigned)entries), dim3(1024), lds, st, pl, table_dev,
              0LL, 0, F, (float2*)nullptr);
    VR_HIP(hipGetLastError());
}

void launch_stft_signals(const FFTPlan& pl, const float* wave, long long L, int hop, int T, int signals, float2* spec, hipStream_t st) {
    prof_note(0.0, (double)signals * (4.0 * (double)L + 8.0 * (double)(pl.n_fft / 2 + 1) * T));
    VR_LAUNCH(stft_kernel, dim3(T, signals), dim3(256), pl.n_fft * sizeof(float2), st, pl, wave, L, hop, T, spec);
    VR_HIP(hipGetLastError());
}

void launch_istft_length(const FFTPlan& pl, const float2* spec, int hop, int T, int signals, float* frames, float* wave, long long length,
                         hipStream_t st) {
    prof_note(0.0, (double)signals * T * (8.0 * (double)(pl.n_fft / 2 + 1) + 4.0 * (double)pl.n_fft));
    VR_LAUNCH(istft_frame_kernel, dim3(T, signals), dim3(256), pl.n_fft * sizeof(float2), st, pl, spec, T, frames);
    VR_HIP(hipGetLastError());
    if (length > 0) {
        prof_note(0.0, (double)signals * (4.0 * (double)T * pl.n_fft + 4.0 * (double)length));
        VR_LAUNCH(istft_ola_kernel, dim3((unsigned)((length + 255) / 256), signals), dim3(256), 0, st, pl, frames, hop, T, length, wave);
        VR_HIP(hipGetLastError());
    }
}

bool istft_masked_available(const FFTPlan& pl, int hop) { return tiled_signal_path(pl, hop); }

void launch_istft(const FFTPlan& pl, const float2* spec, int hop, int T, float* frames, float* wave, hipStream_t st) {
    if (tiled_signal_path(pl, hop)) {
        launch_istft_masked(pl, spec, hop, T, nullptr, 0, nullptr, 0, 0, nullptr, 0, wave, st);
        return;
    }
    VR_LAUNCH(istft_frame_kernel, dim3(T, 2), dim3(256), pl.n_fft * sizeof(float2), st, pl, spec, T, frames);
    VR_HIP(hipGetLastError());
    const long long out_len = (long long)hop * (T - 1);
    if (out_len > 0) {
        VR_LAUNCH(istft_ola_kernel, dim3((unsigned)((out_len + 255) / 256), 2), dim3(256), 0, st, pl, frames,
                           hop, T, out_len, wave);
        VR_HIP(hipGetLastError());
    }
}

// -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ord32(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord32(unsigned o) {
    const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __uint_as_float(u);
}


// ---- spectrogram images (vr_spec_image*, vr_separate_*_img) ---------------------------------------------------------
// lib/spec_utils.py:34-57 in float32 as numpy evaluates it: y = log10(|z|^2 + 1e-8) or angle(z) (a float input: s for |z|, s for the
// angle), lo = min y, r = max (y - lo) = max y - lo (the float32 difference is monotone in y), pixel = uint8((y - lo) * (255 / r)),
// truncated.  Every step is one float32 operation of its own: nothing here is contracted into a fused multiply-add.
template <bool PHASE>
__device__ __forceinline__ float img_y(float2 z) {
#pragma clang fp contract(off)
    if constexpr (PHASE) return atan2f(z.y, z.x);
    const float a = hypotf(z.x, z.y);               // np.abs of a complex64
    const float q = a * a;
    return log10f(q + 1e-8f);
}
template <bool PHASE>
__device__ __forceinline__ float img_y(float s) {
#pragma clang fp contract(off)
    if constexpr (PHASE) return s;
    const float q = s * s;
    return log10f(q + 1e-8f);
}
// r == 0 (a constant input; the reference casts NaN there): zero.  The clamps only keep a NaN or Inf input inside a byte.
__device__ __forceinline__ unsigned img_pixel(float y, float lo, float scale, bool flat) {
#pragma clang fp contract(off)
    const float d = y - lo;
    const float s = d * scale;
    return flat ? 0u : (unsigned)fminf(fmaxf(s, 0.f), 255.f);
}

// What rides behind the arguments of the image forms of mag_pad_kernel (the range pass) and apply_mask_kernel (the write pass).
struct SpecImage { int channels, mode, nparts; };            // SRC = const ImgSeg: stored spectrograms, `src` is the job table
struct StemImage { const ImgSeg* jobs; int nparts; };        // SRC = const SongSeg: the two stems of every song, one job per song

// The two sources.  load(p, y): y[stem][channel] of pixel p = bin * T + frame; consecutive lanes take consecutive p, so every row of
// either channel is read along t.
template <bool CPLX>
struct SpecSource {                                          // complex64 (CPLX) or float32 planes [C][bins * T]
    static constexpr int NS = 1;
    const void* src; long long plane;
    template <bool PHASE, int C>
    __device__ __forceinline__ void load(int p, float (&y)[2][2]) const {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if constexpr (CPLX) y[0][c] = img_y<PHASE>(static_cast<const float2*>(src)[c * plane + p]);
            else y[0][c] = img_y<PHASE>(static_cast<const float*>(src)[c * plane + p]);
        }
    }
};
template <bool CPLX>
struct StemSource {                                          // the float2 apply_mask_kernel would store: the same expressions in the same order
    static constexpr int NS = 2;
    const float2* spec; const float* ma; const float* mb; const float* wgt; int W, T, bins;
    template <bool PHASE, int C>
    __device__ __forceinline__ void load(int p, float (&y)[2][2]) const {
        const int k = p / T, t = p - k * T;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long long row = (long long)c * bins + k;
            const float2 z = spec[row * T + t];
            float2 ys, vs;
            if constexpr (CPLX) {
                const float2 mc = final_mask(reinterpret_cast<const float2*>(ma), W, reinterpret_cast<const float2*>(mb), W, 0, wgt, row, t);
                ys = cmul(mc, z);
                vs = cmul(make_float2(1.f - mc.x, -mc.y), z);
            } else {
                float m = ma[row * W + t];
                if (mb) m = (m + mb[row * W + t]) * 0.5f;
                if (wgt) m += wgt[t] * (1.f - m);
                ys = make_float2(m * z.x, m * z.y);
                const float im = 1.f - m;
                vs = make_float2(im * z.x, im * z.y);
            }
            y[0][c] = img_y<PHASE>(ys);
            y[1][c] = img_y<PHASE>(vs);
        }
    }
};

// (min, max) of four values over the workgroup's 256 threads: the xor butterfly per wave, then the four waves through LDS.  Minimum and
// maximum do not depend on the order, so two calls give the same bits; no atomics.
__device__ __forceinline__ float4 img_reduce(float4 v, float4* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v.x = fminf(v.x, __shfl_xor(v.x, off, 64)); v.y = fmaxf(v.y, __shfl_xor(v.y, off, 64));
        v.z = fminf(v.z, __shfl_xor(v.z, off, 64)); v.w = fmaxf(v.w, __shfl_xor(v.w, off, 64));
    }
    __syncthreads();                                 // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float4 a = red[0], b = red[1], c = red[2], d = red[3];
    return make_float4(fminf(fminf(a.x, b.x), fminf(c.x, d.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y)),
                       fminf(fminf(a.z, b.z), fminf(c.z, d.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w)));
}

// The range pass, grid (parts, job), 256 threads: workgroup b takes the chunks b, b + parts, ... of kImgChunk pixels and leaves its
// (min, max) per stem in part[b]; a workgroup past its job's last chunk leaves (+inf, -inf).
template <bool PHASE, int C, class F>
__device__ __forceinline__ void img_range_pass(const F& f, long long pixels, float4* __restrict__ part) {
    __shared__ float4 red[4];
    float4 m = make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
    for (long long base = (long long)blockIdx.x * kImgChunk; base < pixels; base += (long long)gridDim.x * kImgChunk) {
#pragma unroll
        for (int i = 0; i < kImgChunk / 256; ++i) {
            const long long p = base + i * 256 + threadIdx.x;
            if (p < pixels) {
                float y[2][2];
                f.template load<PHASE, C>((int)p, y);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    m.x = fminf(m.x, y[0][c]); m.y = fmaxf(m.y, y[0][c]);
                    if constexpr (F::NS == 2) { m.z = fminf(m.z, y[1][c]); m.w = fmaxf(m.w, y[1][c]); }
                }
            }
        }
    }
    m = img_reduce(m, red);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// The write pass, grid (pixels of the longest job / (kImgWriteChunks * kImgChunk), job), 256 threads.  Every workgroup reduces the
// job's `nparts` partials again (a few KB from L2), so that no third launch stands between the passes; the first one leaves (lo, r) per
// stem in `range`.  A chunk's pixels are computed with the lanes along t, laid out as bytes in LDS and stored as dwords: a chunk begins
// at a multiple of 4 bytes of the picture whatever T is, so only a picture whose own address is no multiple of 4, and the last bytes
// of the last chunk, go out as bytes.
template <bool PHASE, int C, class F>
__device__ __forceinline__ void img_write_pass(const F& f, long long pixels, const float4* __restrict__ part, int nparts, float* __restrict__ range,
                                               uint8_t* const (&img)[2]) {
    constexpr int NS = F::NS, PB = C == 2 ? 3 : 1;
    __shared__ float4 red[4];
    __shared__ unsigned tile[NS][kImgChunk * PB / 4];
    float4 m = make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const float4 q = part[i];
        m = make_float4(fminf(m.x, q.x), fmaxf(m.y, q.y), fminf(m.z, q.z), fmaxf(m.w, q.w));
    }
    m = img_reduce(m, red);
    float lo[2], r[2], scale[2];
    {
#pragma clang fp contract(off)
        lo[0] = m.x; r[0] = m.y - m.x;
        lo[1] = m.z; r[1] = m.w - m.z;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        scale[s] = (float)(255.0 / (double)r[s]);   // the float32 quotient: a double quotient rounds to it exactly (53 >= 2 * 24 + 2)
        if (blockIdx.x == 0 && threadIdx.x == 0) { range[2 * s] = lo[s]; range[2 * s + 1] = r[s]; }
    }
    for (int cc = 0; cc < kImgWriteChunks; ++cc) {
        const long long base = ((long long)blockIdx.x * kImgWriteChunks + cc) * kImgChunk;
        if (base >= pixels) break;                   // (uniform per workgroup)
#pragma unroll
        for (int i = 0; i < kImgChunk / 256; ++i) {
            const int e = i * 256 + threadIdx.x;
            if (base + e < pixels) {
                float y[2][2];
                f.template load<PHASE, C>((int)(base + e), y);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    uint8_t* tb = reinterpret_cast<uint8_t*>(tile[s]);
                    const unsigned l = img_pixel(y[s][0], lo[s], scale[s], !(r[s] > 0.f));
                    if constexpr (C == 2) {
                        const unsigned rr = img_pixel(y[s][1], lo[s], scale[s], !(r[s] > 0.f));
                        tb[3 * e] = (uint8_t)(l > rr ? l : rr); tb[3 * e + 1] = (uint8_t)l; tb[3 * e + 2] = (uint8_t)rr;
                    } else {
                        tb[e] = (uint8_t)l;
                    }
                }
            }
        }
        __syncthreads();
        const long long left = pixels - base;
        const int nbytes = (int)(left < kImgChunk ? left : kImgChunk) * PB;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            uint8_t* out = img[s] + base * PB;
            const uint8_t* tb = reinterpret_cast<const uint8_t*>(tile[s]);
            if ((reinterpret_cast<uintptr_t>(out) & 3) == 0) {
                for (int d = threadIdx.x; d < nbytes / 4; d += 256) reinterpret_cast<unsigned*>(out)[d] = tile[s][d];
                for (int b = (nbytes & ~3) + threadIdx.x; b < nbytes; b += 256) out[b] = tb[b];
            } else {
                for (int b = threadIdx.x; b < nbytes; b += 256) out[b] = tb[b];
            }
        }
        __syncthreads();
    }
}

// Either pass of either source: the job (blockIdx.y), its source, then the pass.  A job of a separation call is a magnitude picture.
template <bool CPLX, bool WRITE>
__device__ __forceinline__ void spec_image_pass(const ImgSeg* __restrict__ jobs, int bins, const SpecImage a) {
    const ImgSeg jb = jobs[blockIdx.y];
    const long long pixels = (long long)bins * jb.T;
    const SpecSource<CPLX> f{jb.src, pixels};
    uint8_t* const img[2] = {jb.img[0], jb.img[1]};
    auto run = [&](auto phase, auto ch) {
        if constexpr (WRITE) img_write_pass<decltype(phase)::value, decltype(ch)::value>(f, pixels, jb.part, a.nparts, jb.range, img);
        else img_range_pass<decltype(phase)::value, decltype(ch)::value>(f, pixels, jb.part);
    };
    using std::integral_constant;
    if (a.mode) { if (a.channels == 2) run(integral_constant<bool, true>{}, integral_constant<int, 2>{}); else run(integral_constant<bool, true>{}, integral_constant<int, 1>{}); }
    else { if (a.channels == 2) run(integral_constant<bool, false>{}, integral_constant<int, 2>{}); else run(integral_constant<bool, false>{}, integral_constant<int, 1>{}); }
}
template <bool CPLX, bool WRITE>
__device__ __forceinline__ void stem_image_pass(const SongSeg* __restrict__ songs, int bins, const float* __restrict__ ma, int W, const float* __restrict__ mb,
                                                const float* __restrict__ wgt, const StemImage a) {
    const SongSeg sg = songs[blockIdx.y];
    const ImgSeg jb = a.jobs[blockIdx.y];
    ma += (long long)(CPLX ? 2 : 1) * sg.mcol_a;
    if (mb) mb += (long long)(CPLX ? 2 : 1) * sg.mcol_b;
    if (wgt) wgt += sg.frame0;
    const StemSource<CPLX> f{sg.spec, ma, mb, wgt, W, sg.T, bins};
    const long long pixels = (long long)bins * sg.T;
    uint8_t* const img[2] = {jb.img[0], jb.img[1]};
    if constexpr (WRITE) img_write_pass<false, 2>(f, pixels, jb.part, a.nparts, jb.range, img);
    else img_range_pass<false, 2>(f, pixels, jb.part);
}

// One workgroup per (channel, bin) row: |X| into the padded crop source (row-contiguous loads and stores, no 64-bit
// division per element) and the row's two maxima into part[row] -- no atomics; coef_affine_kernel reduces the 2 x bins
// partials.  (Round 1: 16 k same-address atomics and a flat 64-bit index made this 190 us for 34 MB.)
// PACK (complex handles): the same row pass stores the complex row as a real row in plane c and an imaginary row in plane c + 2
// ([re L, re R, im L, im R], lib/nets.py:84 cat([x.real, x.imag], dim=1)), times the complex *scale when given, zero outside
// [pad_l, pad_l + T) (the whole row is written: no pre-zeroing), for blockIdx.y = batch item n; no statistics.
// SRC = const SongSeg, PACK false: the statistics pass per song, blockIdx = (row, song), the row's maxima into part[song][row] and
// no |X| store.  GATHER (song table only; T = cropsize, Wpad = max_bin, part = the crop list as (song, first frame) pairs, scale =
// aff [song][4] holding 1 / c; a StreamSeg entry brings its own): blockIdx = (row of [2][max_bin], crop n); the crop's frames [first, first + cropsize) of its song become
// item n of the dense network input mag_pad [n][nin][max_bin][cropsize] -- |X| / c (PACK false) or the planes [re L, re R, im L, im R]
// of X / c (PACK true), zero outside [0, T_song).  It stands for memset + mag_pad + materialize (+ pack) of the one-song path and for
// its strided crop view, so that a device batch can hold crops of several songs and of both TTA passes.
// IM (at most one type): the range pass of the spectrogram images -- min and max of y per job, grid (parts, job).
// SpecImage (SRC = const ImgSeg, PACK = complex64 input): `spec` is the job table.  StemImage (SRC = const SongSeg, PACK = complex
// mask): the two stems of every song; mag_pad / Wpad / pad_l / scale carry the call's mask, its row pitch, whether the TTA pass is
// averaged in, and the merge_artifacts weights, as apply_mask_kernel takes them.
template <bool PACK, class SRC = const float2, bool GATHER = false, class... IM>
__global__ __launch_bounds__(256) void mag_pad_kernel(SRC* __restrict__ spec, int T, float* __restrict__ mag_pad,
                                                      int Wpad, int pad_l, unsigned long long* __restrict__ part, int bins,
                                                      const float2* __restrict__ scale, IM... im) {
    static_assert(sizeof...(IM) <= 1 && !(sizeof...(IM) && GATHER), "the image forms are forms of their own");
    if constexpr (kHasType<SpecImage, IM...>) {
        spec_image_pass<PACK, false>(spec, bins, pcm_first(im...));
        return;
    } else if constexpr (kHasType<StemImage, IM...>) {
        stem_image_pass<PACK, false>(spec, bins, mag_pad, Wpad, pad_l ? mag_pad : nullptr, reinterpret_cast<const float*>(scale), pcm_first(im...));
        return;
    } else if constexpr (GATHER) {
        const int max_bin = Wpad, cropsize = T;
        const int c = blockIdx.x / max_bin, k = blockIdx.x - c * max_bin, n = blockIdx.y;
        const int2 cr = reinterpret_cast<const int2*>(part)[n];
        const auto sg = spec[cr.x];                                 // (streams: the table entry of the crop's stream)
        const float2* sp;
        if constexpr (kStream<SRC>) sp = sg.ring + ((long long)c * bins + k) * sg.R;
        else sp = sg.spec + ((long long)c * bins + k) * sg.T;
        float* d0 = mag_pad + (((long long)n * (PACK ? 4 : 2) + c) * max_bin + k) * cropsize;
        float* d1 = d0 + 2LL * max_bin * cropsize;                  // (PACK: the imaginary plane)
        float2 s;
        if constexpr (kStream<SRC>) s = *reinterpret_cast<const float2*>(sg.aff);        // 1 / c travels with the entry
        else s = scale[2 * cr.x];
        for (int col = threadIdx.x; col < cropsize; col += 256) {
            const int t = cr.y + col;
            float2 z;
            if constexpr (kStream<SRC>) z = (t >= 0 && t < sg.T) ? sp[t % sg.R] : make_float2(0.f, 0.f);
            else z = (t >= 0 && t < sg.T) ? sp[t] : make_float2(0.f, 0.f);
            if constexpr (PACK) {
                const float2 q = cmul(z, s);
                d0[col] = q.x;
                d1[col] = q.y;
            } else {
                d0[col] = sqrtf(z.x * z.x + z.y * z.y) * s.x;
            }
        }
        return;
    } else if constexpr (PACK) {
        const int row = blockIdx.x, n = blockIdx.y;                  // row = c * bins + k
        const int c = row / bins, k = row - c * bins;
        const float2* sp = spec + ((long long)n * 2 * bins + row) * T;
        float* re = mag_pad + (((long long)n * 4 + c) * bins + k) * Wpad;
        float* im = mag_pad + (((long long)n * 4 + c + 2) * bins + k) * Wpad;
        const float2 s = scale ? *scale : make_float2(1.f, 0.f);
        for (int col = threadIdx.x; col < Wpad; col += 256) {
            const int t = col - pad_l;
            float2 z = (t >= 0 && t < T) ? sp[t] : make_float2(0.f, 0.f);
            if (scale) z = cmul(z, s);
            re[col] = z.x;
            im[col] = z.y;
        }
        return;
    }
    int row = blockIdx.x;
    const float2* sp;
    float* dst = nullptr;
    int t_first = 0, ring = 0;                       // (stream) the new frames [t_new, T) at column t % R; the maxima join part[row]
    if constexpr (kStream<SRC>) {
        const StreamSeg sg = spec[0];
        T = sg.T; t_first = sg.t_new; ring = sg.R;
        sp = sg.ring + (long long)row * ring;
    } else if constexpr (kSongTable<SRC>) {
        const SongSeg sg = spec[blockIdx.y];
        T = sg.T;
        sp = sg.spec + (long long)row * T;
        row += blockIdx.y * 2 * bins;
    } else if constexpr (sizeof...(IM) == 0) {
        sp = spec + (long long)row * T;
        dst = mag_pad + (long long)row * Wpad + pad_l;
    }
    float mx = 0.f;
    unsigned long long key = ((unsigned long long)ord32(0.f) << 32) | ord32(0.f);   // the zero padding is part of the reduced array
    for (int t = t_first + threadIdx.x; t < T; t += 256) {
        float2 z;
        if constexpr (kStream<SRC>) z = sp[t % ring];
        else z = sp[t];
        const float m = sqrtf(z.x * z.x + z.y * z.y);
        if constexpr (!kSongTable<SRC> && !kStream<SRC>) dst[t] = m;
        mx = fmaxf(mx, m);
        // numpy compares -0.0 == +0.0 and goes on to the imaginary part; as bit patterns -0.0 would sort below the padding's +0.0
        const unsigned long long k = ((unsigned long long)ord32(z.x + 0.f) << 32) | ord32(z.y + 0.f);
        key = k > key ? k : key;
    }
    __shared__ float rmx[4];
    __shared__ unsigned long long rkey[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) { rmx[threadIdx.x >> 6] = mx; rkey[threadIdx.x >> 6] = key; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) { mx = fmaxf(mx, rmx[i]); key = rkey[i] > key ? rkey[i] : key; }
        if constexpr (kStream<SRC>) {
            mx = fmaxf(mx, __uint_as_float((unsigned)part[2 * row]));
            key = part[2 * row + 1] > key ? part[2 * row + 1] : key;
        }
        part[2 * row] = (unsigned long long)__float_as_uint(mx);
        part[2 * row + 1] = key;
    }
}

void launch_mag_pad(const float2* spec, int bins, int T, float* mag_pad, int Wpad, int pad_l, unsigned* stats,
                    hipStream_t st) {
    prof_note(0.0, 2.0 * (double)bins * (8.0 * T + 4.0 * Wpad));
    VR_LAUNCH((mag_pad_kernel<false>), dim3(2 * bins), dim3(256), 0, st, spec, T, mag_pad, Wpad, pad_l,
                       reinterpret_cast<unsigned long long*>(stats) + 2, bins, nullptr);
    VR_HIP(hipGetLastError());
}

// stats layout: a 16-byte header, then 2 x bins rows of (max |X| bits, lexicographic complex key) partials
// CPLX (complex handles): aff[0..1] = 1 / c as a complex number, formed in double and rounded once -- c = max|X| (mode 0,
// inference.py:74) or the lexicographic complex maximum itself (mode 1, inference.py:87,94: numpy divides by the complex number,
// which also rotates the phase)
// PER_SONG: blockIdx.x = song, stats = that layout without the header for every song ([song][rows] partials), aff [song][4]
// The one-song forms also leave what they reduced in the 16-byte header: (max |X| bits, the selected key) -- read by the tests only.
template <bool CPLX, bool PER_SONG = false>
__global__ __launch_bounds__(256) void coef_affine_kernel(unsigned* stats, int rows, int mode, float* aff) {
    const unsigned long long* part = reinterpret_cast<unsigned long long*>(stats) + 2;
    if constexpr (PER_SONG) {
        part = reinterpret_cast<unsigned long long*>(stats) + (long long)blockIdx.x * rows * 2;
        aff += 4 * blockIdx.x;
    }
    unsigned mxb = 0u;
    unsigned long long key = ((unsigned long long)ord32(0.f) << 32) | ord32(0.f);
    for (int r = threadIdx.x; r < rows; r += 256) {
        const unsigned b = (unsigned)part[2 * r];
        mxb = b > mxb ? b : mxb;                               // non-negative floats order like their bit patterns
        key = part[2 * r + 1] > key ? part[2 * r + 1] : key;
    }
    __shared__ unsigned rm[256];
    __shared__ unsigned long long rk[256];
    rm[threadIdx.x] = mxb; rk[threadIdx.x] = key;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            rm[threadIdx.x] = rm[threadIdx.x + off] > rm[threadIdx.x] ? rm[threadIdx.x + off] : rm[threadIdx.x];
            rk[threadIdx.x] = rk[threadIdx.x + off] > rk[threadIdx.x] ? rk[threadIdx.x + off] : rk[threadIdx.x];
        }
        __syncthreads();
    }
    if constexpr (!PER_SONG) {
        if (threadIdx.x == 0) {
            reinterpret_cast<unsigned long long*>(stats)[0] = rm[0];
            reinterpret_cast<unsigned long long*>(stats)[1] = rk[0];
        }
    }
    if constexpr (CPLX) {
        if (threadIdx.x == 0) {
            double re = (double)__uint_as_float(rm[0]), im = 0.0;
            if (mode != 0) {
                re = (double)unord32((unsigned)(rk[0] >> 32));
                im = (double)unord32((unsigned)(rk[0] & 0xffffffffu));
            }
            const double n2 = re * re + im * im;
            aff[0] = (float)(re / n2); aff[1] = (float)(-im / n2);
        }
        return;
    }
    if (threadIdx.x == 0) {
        float coef;
        if (mode == 0) {
            coef = __uint_as_float(rm[0]);
        } else {
            const float re = unord32((unsigned)(rk[0] >> 32)), im = unord32((unsigned)(rk[0] & 0xffffffffu));
            coef = sqrtf(re * re + im * im);
        }
        const float s = 1.f / coef;
        aff[0] = s; aff[1] = 0.f; aff[2] = s; aff[3] = 0.f;
    }
}
void launch_coef_affine(unsigned* stats, int rows, int mode, float* aff, hipStream_t st) {
    VR_LAUNCH((coef_affine_kernel<false>), dim3(1), dim3(256), 0, st, stats, rows, mode, aff);
    VR_HIP(hipGetLastError());
}

void launch_coef_complex(unsigned* stats, int rows, int mode, float2* inv, hipStream_t st) {
    VR_LAUNCH((coef_affine_kernel<true>), dim3(1), dim3(256), 0, st, stats, rows, mode, reinterpret_cast<float*>(inv));
    VR_HIP(hipGetLastError());
}

void launch_pack_complex(const float2* spec, int N, int bins, int T, float* dst, int Wdst, int pad_l, const float2* scale,
                         hipStream_t st) {
    prof_note(0.0, (double)N * 2 * bins * (8.0 * T + 8.0 * Wdst));
    VR_LAUNCH((mag_pad_kernel<true>), dim3(2 * bins, N), dim3(256), 0, st, spec, T, dst, Wdst, pad_l, nullptr, bins, scale);
    VR_HIP(hipGetLastError());
}

// per-frame minimum of the final mask over (channel, bin): input of spec_utils.merge_artifacts
// (lib/spec_utils.py:64).  One workgroup per 64 frames; lanes along time (coalesced rows).
// CPLX: complex64 masks, the minimum of |mask| (inference.py:28-29)
// DST = const SongSeg: `dst` is the song table, blockIdx.y = song, the minima go to that song's own fmin
constexpr int kStreamMinFrames = 8;       // frames per workgroup of the stream form's minima
template <bool CPLX, class DST = float>
__global__ __launch_bounds__(256) void frame_min_kernel(int rows, int T, const float* __restrict__ ma, int Wa,
                                                        const float* __restrict__ mb, int Wb, int shift,
                                                        DST* __restrict__ dst) {
    __shared__ float red[4][64];
    float* __restrict__ fmin;
    if constexpr (kStream<DST>) {
        // DST = const StreamSeg (--postprocess streams): blockIdx.y = table entry; an entry without the rings is skipped.
        // rows > 0: the minima of the entry's frames [fm_lo, fm_hi) from its mask rings (pass 0 at column t % RM, the TTA pass at
        // (t + shift) % RM, averaged as the masked iSTFT averages them) into fmin_ring[t % RW]; T, ma .. shift are unused.
        // rows == 0: the walk -- one workgroup per entry takes those minima through stream_post_advance (stream_post.h): the wave
        // brings them into LDS, lane 0 walks the state and stores the weights; no atomics, nothing comes back to the host.
        const StreamSeg sg = dst[blockIdx.y];
        if (!sg.fmin_ring) return;
        if (rows == 0) {
            __shared__ float fm[1024];
            if (blockIdx.x) return;
            StreamPostState ps = *sg.post;
            for (int base = ps.h; base < sg.fm_hi; base += 1024) {
                const int n = sg.fm_hi - base < 1024 ? sg.fm_hi - base : 1024;
                for (int i = threadIdx.x; i < n; i += 256) fm[i] = sg.fmin_ring[(base + i) % sg.RW];
                __syncthreads();
                if (threadIdx.x == 0) stream_post_advance(ps, fm, n, sg.wgt_ring, sg.RW);
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (sg.post_flush) stream_post_finish(ps, sg.wgt_ring, sg.RW);
                *sg.post = ps;
            }
            return;
        }
        // (a step brings few frames -- one crop's roi in a steady push -- so a workgroup takes kStreamMinFrames of them and splits the rows
        // 256 / kStreamMinFrames ways: 64 frames per workgroup, as offline, would leave a steady push to two workgroups)
        constexpr int FW = kStreamMinFrames, PARTS = 256 / FW;
        if ((int)blockIdx.x * FW >= sg.fm_hi - sg.fm_lo) return;
        const int fl = threadIdx.x % FW, part = threadIdx.x / FW;
        const int t = sg.fm_lo + blockIdx.x * FW + fl;
        const int ca = t % sg.RM, cb = (t + sg.shift) % sg.RM;
        float* redf = &red[0][0];                           // [PARTS][FW]
        float m = 3.4e38f;
        if (t < sg.fm_hi) {
            for (int r = part; r < rows; r += PARTS) {
                if constexpr (CPLX) {
                    float2 v = reinterpret_cast<const float2*>(sg.mask_a)[(long long)r * sg.RM + ca];
                    if (sg.mask_b) {
                        const float2 b = reinterpret_cast<const float2*>(sg.mask_b)[(long long)r * sg.RM + cb];
                        v = make_float2((v.x + b.x) * 0.5f, (v.y + b.y) * 0.5f);
                    }
                    m = fminf(m, hypotf(v.x, v.y));
                } else {
                    float v = sg.mask_a[(long long)r * sg.RM + ca];
                    if (sg.mask_b) v = (v + sg.mask_b[(long long)r * sg.RM + cb]) * 0.5f;
                    m = fminf(m, v);
                }
            }
        }
        redf[threadIdx.x] = m;
        __syncthreads();
        if (part == 0 && t < sg.fm_hi) {
            for (int q = 1; q < PARTS; ++q) m = fminf(m, redf[q * FW + fl]);
            sg.fmin_ring[t % sg.RW] = m;
        }
        return;
    } else if constexpr (kSongTable<DST>) {
        const SongSeg sg = dst[blockIdx.y];
        T = sg.T;
        ma += (long long)(CPLX ? 2 : 1) * sg.mcol_a;
        if (mb) mb += (long long)(CPLX ? 2 : 1) * sg.mcol_b;
        fmin = sg.fmin;
    } else {
        fmin = dst;
    }
    const int t = blockIdx.x * 64 + (threadIdx.x & 63);
    const int part = threadIdx.x >> 6;
    float m = 3.4e38f;
    if (t < T) {
        for (int r = part; r < rows; r += 4) {
            if constexpr (CPLX) {
                const float2 v = final_mask(reinterpret_cast<const float2*>(ma), Wa, reinterpret_cast<const float2*>(mb), Wb, shift,
                                            nullptr, r, t);
                m = fminf(m, hypotf(v.x, v.y));
            } else {
                float v = ma[(long long)r * Wa + t];
                if (mb) v = (v + mb[(long long)r * Wb + t + shift]) * 0.5f;
                m = fminf(m, v);
            }
        }
    }
    red[part][threadIdx.x & 63] = m;
    __syncthreads();
    if (part == 0 && t < T) fmin[t] = fminf(fminf(red[0][threadIdx.x], red[1][threadIdx.x]), fminf(red[2][threadIdx.x], red[3][threadIdx.x]));
}

void launch_frame_min(int bins, int T, const float* mask_a, int Wa, const float* mask_b, int Wb, int shift, float* fmin,
                      hipStream_t st) {
    VR_LAUNCH((frame_min_kernel<false>), dim3((T + 63) / 64), dim3(256), 0, st, 2 * bins, T, mask_a, Wa, mask_b, Wb, shift, fmin);
    VR_HIP(hipGetLastError());
}

// ---- the pseudo-label back end (vr_pseudo*) ---------------------------------------------------------------------
// the instruments stem of apply_mask_kernel at (row, t) for the spectrogram value z: the same expressions in the same order
template <bool CPLX>
__device__ __forceinline__ float2 instruments_stem(const float* __restrict__ ma, int Wa, const float* __restrict__ mb, int Wb, int shift,
                                                   const float* __restrict__ wgt, long long row, int t, float2 z) {
    if constexpr (CPLX) {
        const float2 mc = final_mask(reinterpret_cast<const float2*>(ma), Wa, reinterpret_cast<const float2*>(mb), Wb, shift, wgt, row, t);
        return cmul(mc, z);
    } else {
        float m = ma[row * Wa + t];
        if (mb) m = (m + mb[row * Wb + t + shift]) * 0.5f;
        if (wgt) m += wgt[t] * (1.f - m);            // merge_artifacts: y_mask += weight * (1 - y_mask)
        return make_float2(m * z.x, m * z.y);
    }
}

// What rides behind apply_mask_kernel's arguments in its pseudo forms: the PseudoSeg table; the type is the layout of `out`.
struct PseudoSpec { const PseudoSeg* ps; };          // VR_PSEUDO_SPEC [2][bins][T]: today's mapping, consecutive lanes along t
struct PseudoRows { const PseudoSeg* ps; };          // VR_PSEUDO_ROWS [T][2][bins]: through an LDS tile
struct PseudoDiff { const PseudoSeg* ps; };          // not a back end: D = X - Y of a spectrogram-level call (pseudo_diff below)
constexpr int PT = 64;                               // the rows form's tile: PT frames x PT bins of one channel
// Row pitch of the tile in float2: lanes along t write a row (kk fixed, consecutive 8-byte addresses: no conflict at any pitch); lanes along
// the bin read a column, lane l at dword 2 * (l * pitch + tt) -- ds_read_b64 banks are (a / 4) % 64 per 32-lane half, so the 32 lanes of a half
// must hit 32 distinct even banks: 2 * l * pitch mod 64 distinct for l < 32, which holds exactly for an odd pitch.  64 would be 32-way.
constexpr int PT_PITCH = PT + 1;

// out = Y + instruments stem of D and nothing else.  SPEC: grid (elements / 256, song) as the plain table form.  ROWS: grid (frame tiles,
// bin tiles x channel, song), 256 threads; the tile is read along t (mask, D, Y rows coalesced), written along the bin (out rows coalesced).
// Edge tiles are masked: no read or write outside [0, T) x [0, bins).
template <bool CPLX, bool ROWS>
__device__ __forceinline__ void pseudo_apply(const SongSeg* __restrict__ songs, const PseudoSeg* __restrict__ pst, int bins,
                                             const float* __restrict__ ma, int Wa, const float* __restrict__ mb, int Wb, int shift,
                                             const float* __restrict__ wgt) {
    const SongSeg sg = songs[ROWS ? blockIdx.z : blockIdx.y];
    const PseudoSeg ps = pst[ROWS ? blockIdx.z : blockIdx.y];
    const int T = sg.T;
    ma += (long long)(CPLX ? 2 : 1) * sg.mcol_a;
    if (mb) mb += (long long)(CPLX ? 2 : 1) * sg.mcol_b;
    if (wgt) wgt += sg.frame0;
    if constexpr (!ROWS) {
        const long long total = 2LL * bins * T;
        const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (gid >= total) return;
        const int t = (int)(gid % T);
        const long long row = gid / T;
        ps.out[gid] = add_rounded(ps.inst[gid], instruments_stem<CPLX>(ma, Wa, mb, Wb, shift, wgt, row, t, sg.spec[gid]));
    } else {
        __shared__ float2 tl[PT * PT_PITCH];
        const int t0 = blockIdx.x * PT;
        if (t0 >= T) return;                         // (the grid is sized for the longest song; uniform per workgroup)
        const int ch = blockIdx.y & 1, k0 = (blockIdx.y >> 1) * PT;
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        {
            const int t = t0 + lane;
            for (int kk = w; kk < PT; kk += 4) {
                const int k = k0 + kk;
                if (k < bins && t < T) {
                    const long long row = (long long)ch * bins + k;
                    const long long e = row * T + t;
                    tl[kk * PT_PITCH + lane] = add_rounded(ps.inst[e], instruments_stem<CPLX>(ma, Wa, mb, Wb, shift, wgt, row, t, sg.spec[e]));
                }
            }
        }
        __syncthreads();
        const int k = k0 + lane;
        for (int tt = w; tt < PT; tt += 4) {
            const int t = t0 + tt;
            if (k < bins && t < T) ps.out[((long long)t * 2 + ch) * bins + k] = tl[lane * PT_PITCH + tt];
        }
    }
}

// D = X - Y over the song table (the pair front end of a spectrogram-level call): blockIdx = (row of [2][bins], song), 256 threads; the
// row's 64-bit offset is formed once, the lanes stream it; no atomics
__device__ __forceinline__ void pseudo_diff(const SongSeg* __restrict__ songs, const PseudoSeg* __restrict__ pst) {
    const SongSeg sg = songs[blockIdx.y];
    const PseudoSeg ps = pst[blockIdx.y];
    const long long base = (long long)blockIdx.x * sg.T;
    const float2* __restrict__ x = ps.mix + base;
    const float2* __restrict__ y = ps.inst + base;
    float2* __restrict__ d = sg.spec + base;
    for (int t = threadIdx.x; t < sg.T; t += 256) d[t] = sub_rounded(x[t], y[t]);
}

// CPLX: complex64 masks, complex products (final_mask: TTA average and merge_artifacts blend of a complex mask)
// PS (at most one type, SRC = const SongSeg): PseudoSpec / PseudoRows = the pseudo back ends above, PseudoDiff = the elementwise pair front
// end -- under this kernel's name, like every form of this file, so that the launch profiler's report keeps one name per stage;
// SpecImage (SRC = const ImgSeg) / StemImage = the write pass of the spectrogram images
template <bool CPLX, class SRC = const float2, class... PS>
__global__ void apply_mask_kernel(SRC* __restrict__ src, int bins, int T, const float* __restrict__ ma,
                                  int Wa, const float* __restrict__ mb, int Wb, int shift, const float* __restrict__ wgt,
                                  float2* __restrict__ y, float2* __restrict__ v, PS... ps) {
    static_assert(sizeof...(PS) <= 1 && (sizeof...(PS) == 0 || kSongTable<SRC> || kHasType<SpecImage, PS...>), "the pseudo forms are song-table forms");
    if constexpr (kHasType<SpecImage, PS...>) {      // the write pass of the spectrogram images (CPLX: complex64 input), src = the job table
        spec_image_pass<CPLX, true>(src, bins, pcm_first(ps...));
        return;
    } else if constexpr (kHasType<StemImage, PS...>) {
        stem_image_pass<CPLX, true>(src, bins, ma, Wa, mb, wgt, pcm_first(ps...));
        return;
    } else if constexpr (kHasType<PseudoDiff, PS...>) {
        pseudo_diff(src, pcm_first(ps...).ps);
        return;
    } else if constexpr (sizeof...(PS) == 1) {
        pseudo_apply<CPLX, kHasType<PseudoRows, PS...>>(src, pcm_first(ps...).ps, bins, ma, Wa, mb, Wb, shift, wgt);
        return;
    }
    const float2* __restrict__ spec;
    if constexpr (kSongTable<SRC>) {                 // blockIdx.y = song, its own y / v
        const SongSeg sg = src[blockIdx.y];
        spec = sg.spec; T = sg.T; y = sg.y; v = sg.v;
        ma += (long long)(CPLX ? 2 : 1) * sg.mcol_a;
        if (mb) mb += (long long)(CPLX ? 2 : 1) * sg.mcol_b;
        if (wgt) wgt += sg.frame0;
    } else if constexpr (sizeof...(PS) == 0) {
        spec = src;
    }
    const long long total = 2LL * bins * T;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int t = (int)(gid % T);
    const long long row = gid / T;
    if constexpr (CPLX) {
        const float2 mc = final_mask(reinterpret_cast<const float2*>(ma), Wa, reinterpret_cast<const float2*>(mb), Wb, shift, wgt,
                                     row, t);
        const float2 zc = spec[gid];
        y[gid] = cmul(mc, zc);
        v[gid] = cmul(make_float2(1.f - mc.x, -mc.y), zc);
        return;
    }
    float m = ma[row * Wa + t];
    if (mb) m = (m + mb[row * Wb + t + shift]) * 0.5f;
    if (wgt) m += wgt[t] * (1.f - m);            // merge_artifacts: y_mask += weight * (1 - y_mask)
    const float2 z = spec[gid];
    y[gid] = make_float2(m * z.x, m * z.y);
    const float im = 1.f - m;
    v[gid] = make_float2(im * z.x, im * z.y);
}

void launch_apply_mask(const float2* spec, int bins, int T, const float* mask_a, int Wa, const float* mask_b, int Wb,
                       int shift, const float* wgt, float2* y, float2* v, hipStream_t st) {
    const long long total = 2LL * bins * T;
    VR_LAUNCH((apply_mask_kernel<false>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, spec, bins, T, mask_a,
                       Wa, mask_b, Wb, shift, wgt, y, v);
    VR_HIP(hipGetLastError());
}

// ---- complex64 masks (is_complex handles) ------------------------------------------------------------
void launch_frame_min_complex(int bins, int T, const float2* mask_a, int Wa, const float2* mask_b, int Wb, int shift, float* fmin,
                              hipStream_t st) {
    VR_LAUNCH((frame_min_kernel<true>), dim3((T + 63) / 64), dim3(256), 0, st, 2 * bins, T, reinterpret_cast<const float*>(mask_a), Wa,
              reinterpret_cast<const float*>(mask_b), Wb, shift, fmin);
    VR_HIP(hipGetLastError());
}

void launch_apply_mask_complex(const float2* spec, int bins, int T, const float2* mask_a, int Wa, const float2* mask_b, int Wb,
                               int shift, const float* wgt, float2* y, float2* v, hipStream_t st) {
    const long long total = 2LL * bins * T;
    VR_LAUNCH((apply_mask_kernel<true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, spec, bins, T,
              reinterpret_cast<const float*>(mask_a), Wa, reinterpret_cast<const float*>(mask_b), Wb, shift, wgt, y, v);
    VR_HIP(hipGetLastError());
}

// ---- many songs in one call (vr_separate_many / vr_separate_wave_many): the SEG instantiations --------------------------------
// Every launch covers all songs of the call: the song is a grid dimension sized for the longest one.
bool many_tiled_available(const FFTPlan& pl, int hop) { return tiled_signal_path(pl, hop); }

void launch_stft_many(const FFTPlan& pl, const SongSeg* songs, int n_songs, int max_T, double sum_L, double sum_T, hipStream_t st,
                      const PcmIn* pcm, double pcm_bytes) {
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    if (pcm) {                                           // the songs' sample bytes, one PcmIn per song beside the table
        static std::atomic<unsigned long long> attr_pcm{0};
        ensure_lds_attr(attr_pcm, reinterpret_cast<const void*>(stft_tile_kernel<const SongSeg, const PcmIn*>), 160 * 1024);
        prof_note(0.0, pcm_bytes + 2.0 * 8.0 * (double)bins * sum_T);
        VR_LAUNCH((stft_tile_kernel<const SongSeg, const PcmIn*>), dim3((unsigned)((max_T + F - 1) / F), 2, n_songs), dim3(1024), lds, st, pl, songs, 0LL,
                  0, F, (float2*)nullptr, pcm);
        VR_HIP(hipGetLastError());
        return;
    }
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const SongSeg>), 160 * 1024);
    prof_note(0.0, 2.0 * (4.0 * sum_L + 8.0 * (double)bins * sum_T));
    VR_LAUNCH((stft_tile_kernel<const SongSeg>), dim3((unsigned)((max_T + F - 1) / F), 2, n_songs), dim3(1024), lds, st, pl, songs, 0LL, 0, F, nullptr);
    VR_HIP(hipGetLastError());
}

void launch_song_stats(const SongSeg* songs, int n_songs, int bins, double sum_T, unsigned long long* part, hipStream_t st) {
    prof_note(0.0, 2.0 * (double)bins * 8.0 * sum_T);
    VR_LAUNCH((mag_pad_kernel<false, const SongSeg>), dim3(2 * bins, n_songs), dim3(256), 0, st, songs, 0, nullptr, 0, 0, part, bins, nullptr);
    VR_HIP(hipGetLastError());
}

void launch_song_coef(const unsigned long long* part, int n_songs, int rows, int mode, bool cplx, float* aff, hipStream_t st) {
    unsigned* stats = reinterpret_cast<unsigned*>(const_cast<unsigned long long*>(part));      // (read only in the per-song form)
    if (cplx) VR_LAUNCH((coef_affine_kernel<true, true>), dim3(n_songs), dim3(256), 0, st, stats, rows, mode, aff);
    else VR_LAUNCH((coef_affine_kernel<false, true>), dim3(n_songs), dim3(256), 0, st, stats, rows, mode, aff);
    VR_HIP(hipGetLastError());
}

void launch_crop_gather(const SongSeg* songs, const int2* crops, int count, bool cplx, int bins, int max_bin, int cropsize, const float* aff,
                        float* dst, hipStream_t st) {
    prof_note(0.0, (double)count * 2 * max_bin * cropsize * (8.0 + (cplx ? 8.0 : 4.0)));
    // (the kernel's T / Wpad / part / scale slots carry cropsize / max_bin / the crop list / aff: see mag_pad_kernel)
    unsigned long long* list = reinterpret_cast<unsigned long long*>(const_cast<int2*>(crops));
    const float2* inv = reinterpret_cast<const float2*>(aff);
    if (cplx) VR_LAUNCH((mag_pad_kernel<true, const SongSeg, true>), dim3(2 * max_bin, count), dim3(256), 0, st, songs, cropsize, dst, max_bin, 0, list, bins, inv);
    else VR_LAUNCH((mag_pad_kernel<false, const SongSeg, true>), dim3(2 * max_bin, count), dim3(256), 0, st, songs, cropsize, dst, max_bin, 0, list, bins, inv);
    VR_HIP(hipGetLastError());
}

void launch_frame_min_many(const SongSeg* songs, int n_songs, int max_T, int bins, const float* mask, int W, int tta, bool cplx,
                           hipStream_t st) {
    const dim3 grid((max_T + 63) / 64, n_songs);
    const float* mb = tta ? mask : nullptr;
    if (cplx) VR_LAUNCH((frame_min_kernel<true, const SongSeg>), grid, dim3(256), 0, st, 2 * bins, 0, mask, W, mb, W, 0, songs);
    else VR_LAUNCH((frame_min_kernel<false, const SongSeg>), grid, dim3(256), 0, st, 2 * bins, 0, mask, W, mb, W, 0, songs);
    VR_HIP(hipGetLastError());
}

void launch_apply_mask_many(const SongSeg* songs, int n_songs, int max_T, int bins, const float* mask, int W, int tta, bool cplx,
                            const float* wgt, hipStream_t st) {
    const long long total = 2LL * bins * max_T;
    const dim3 grid((unsigned)((total + 255) / 256), n_songs);
    const float* mb = tta ? mask : nullptr;
    if (cplx) VR_LAUNCH((apply_mask_kernel<true, const SongSeg>), grid, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, nullptr, nullptr);
    else VR_LAUNCH((apply_mask_kernel<false, const SongSeg>), grid, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, nullptr, nullptr);
    VR_HIP(hipGetLastError());
}

void launch_istft_masked_many(const FFTPlan& pl, const SongSeg* songs, int n_songs, int max_T, double sum_T, const float* mask, int W, int tta,
                              bool cplx, const float* wgt, int which, hipStream_t st, bool pcm16) {
    const int M = pl.n_fft / 2, bins = M + 1;
    if (max_T < 2) return;
    const int F = tile_frames(pl, M);
    const int S = F - 1;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8 + (size_t)M * 4;
    const dim3 grid((unsigned)((max_T - 1 + S - 1) / S), 2, n_songs);
    prof_note(0.0, 2.0 * ((double)bins * sum_T * (8.0 + (cplx ? 8.0 : 4.0) * (tta ? 2 : 1)) + (pcm16 ? 2.0 : 4.0) * (double)M * sum_T));
    const float* mb = tta ? mask : nullptr;
    if (pcm16) {                                         // y_wave / v_wave of the table point to interleaved int16
        if (cplx) {
            static std::atomic<unsigned long long> attr_done{0};
            ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<true, const SongSeg, WavePcm16Out>), 160 * 1024);
            VR_LAUNCH((istft_tile_kernel<true, const SongSeg, WavePcm16Out>), grid, dim3(1024), lds, st, pl, songs, 0, S, mask, W, mb, W, 0, wgt, which, nullptr, 0LL);
        } else {
            static std::atomic<unsigned long long> attr_done{0};
            ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<false, const SongSeg, WavePcm16Out>), 160 * 1024);
            VR_LAUNCH((istft_tile_kernel<false, const SongSeg, WavePcm16Out>), grid, dim3(1024), lds, st, pl, songs, 0, S, mask, W, mb, W, 0, wgt, which, nullptr, 0LL);
        }
        VR_HIP(hipGetLastError());
        return;
    }
    if (cplx) {
        static std::atomic<unsigned long long> attr_done{0};
        ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<true, const SongSeg>), 160 * 1024);
        VR_LAUNCH((istft_tile_kernel<true, const SongSeg>), grid, dim3(1024), lds, st, pl, songs, 0, S, mask, W, mb, W, 0, wgt, which, nullptr, 0LL);
    } else {
        static std::atomic<unsigned long long> attr_done{0};
        ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<false, const SongSeg>), 160 * 1024);
        VR_LAUNCH((istft_tile_kernel<false, const SongSeg>), grid, dim3(1024), lds, st, pl, songs, 0, S, mask, W, mb, W, 0, wgt, which, nullptr, 0LL);
    }
    VR_HIP(hipGetLastError());
}

// ---- pseudo-instrument labels (vr_pseudo*) -----------------------------------------------------------------------
void launch_stft_pseudo_many(const FFTPlan& pl, const SongSeg* songs, const PseudoSeg* ps, int n_songs, int max_T, double sum_L, double sum_T,
                             hipStream_t st) {
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const SongSeg, const PseudoSeg*>), 160 * 1024);
    prof_note(0.0, 2.0 * 2.0 * (4.0 * sum_L + 8.0 * (double)bins * sum_T));         // two waves read, Y and D written
    VR_LAUNCH((stft_tile_kernel<const SongSeg, const PseudoSeg*>), dim3((unsigned)((max_T + F - 1) / F), 2, n_songs), dim3(1024), lds, st, pl, songs, 0LL,
              0, F, (float2*)nullptr, ps);
    VR_HIP(hipGetLastError());
}

void launch_pseudo_diff_many(const SongSeg* songs, const PseudoSeg* ps, int n_songs, int bins, double sum_T, hipStream_t st) {
    prof_note(0.0, 2.0 * (double)bins * 24.0 * sum_T);
    VR_LAUNCH((apply_mask_kernel<false, const SongSeg, PseudoDiff>), dim3(2 * bins, n_songs), dim3(256), 0, st, songs, bins, 0, (const float*)nullptr, 0,
              (const float*)nullptr, 0, 0, (const float*)nullptr, (float2*)nullptr, (float2*)nullptr, PseudoDiff{ps});
    VR_HIP(hipGetLastError());
}

void launch_apply_mask_pseudo_many(const SongSeg* songs, const PseudoSeg* ps, int n_songs, int max_T, int bins, const float* mask, int W, int tta,
                                   bool cplx, const float* wgt, bool rows, double sum_T, hipStream_t st) {
    const float* mb = tta ? mask : nullptr;
    prof_note(0.0, 2.0 * (double)bins * sum_T * (24.0 + (cplx ? 8.0 : 4.0) * (tta ? 2 : 1)));          // D, Y read, P written, the mask(s)
    if (rows) {
        const dim3 grid((max_T + PT - 1) / PT, 2 * ((bins + PT - 1) / PT), n_songs);
        const PseudoRows a{ps};
        if (cplx) VR_LAUNCH((apply_mask_kernel<true, const SongSeg, PseudoRows>), grid, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, nullptr, nullptr, a);
        else VR_LAUNCH((apply_mask_kernel<false, const SongSeg, PseudoRows>), grid, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, nullptr, nullptr, a);
    } else {
        const long long total = 2LL * bins * max_T;
        const dim3 grid((unsigned)((total + 255) / 256), n_songs);
        const PseudoSpec a{ps};
        if (cplx) VR_LAUNCH((apply_mask_kernel<true, const SongSeg, PseudoSpec>), grid, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, nullptr, nullptr, a);
        else VR_LAUNCH((apply_mask_kernel<false, const SongSeg, PseudoSpec>), grid, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, nullptr, nullptr, a);
    }
    VR_HIP(hipGetLastError());
}

// ---- evaluation (vr_evaluate_wave*) ---------------------------------------------------------------------------
size_t eval_part_doubles(int T) { return T < 2 ? 0 : (size_t)2 * 2 * (T - 1) * 4 * 4; }

int eval_tile_step(const FFTPlan& pl) { return tile_frames(pl, pl.n_fft / 2) - 1; }

void launch_istft_eval_many(const FFTPlan& pl, const SongSeg* songs, const WaveEval* evs, int n_songs, int max_T, double sum_T, const float* mask_a,
                            int Wa, const float* mask_b, int Wb, int shift, bool cplx, const float* wgt, int which, bool stored, hipStream_t st) {
    const int M = pl.n_fft / 2, bins = M + 1;
    if (max_T < 2) return;
    const int F = tile_frames(pl, M);
    const int S = F - 1;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8 + (size_t)M * 4;
    const dim3 grid((unsigned)((max_T - 1 + S - 1) / S), 2, n_songs);
    // the plain form's traffic with the stem written only if stored; the true stem (which 1: and the mixture) read, the partials written
    prof_note(0.0, 2.0 * ((double)bins * sum_T * (8.0 + (cplx ? 8.0 : 4.0) * (mask_b ? 2 : 1)) + ((stored ? 4.0 : 0.0) + (which ? 8.0 : 4.0)) * (double)M * sum_T
                          + 128.0 * sum_T));
    float* ev = reinterpret_cast<float*>(const_cast<WaveEval*>(evs));       // (the table forms do not read `wave`: the entries ride there)
    if (cplx) {
        static std::atomic<unsigned long long> attr_done{0};
        ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<true, const SongSeg, const WaveEval*>), 160 * 1024);
        VR_LAUNCH((istft_tile_kernel<true, const SongSeg, const WaveEval*>), grid, dim3(1024), lds, st, pl, songs, 0, S, mask_a, Wa, mask_b, Wb, shift, wgt, which, ev, 0LL);
    } else {
        static std::atomic<unsigned long long> attr_done{0};
        ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<false, const SongSeg, const WaveEval*>), 160 * 1024);
        VR_LAUNCH((istft_tile_kernel<false, const SongSeg, const WaveEval*>), grid, dim3(1024), lds, st, pl, songs, 0, S, mask_a, Wa, mask_b, Wb, shift, wgt, which, ev, 0LL);
    }
    VR_HIP(hipGetLastError());
}

void launch_eval_sums(const FFTPlan& pl, const SongSeg* songs, const WaveEval* evs, int n_songs, long long max_windows, double sum_T, hipStream_t st) {
    if (max_windows <= 0) return;
    VR_CHECK(max_windows < (1LL << 31), -2, "too many windows for one call");
    prof_note(0.0, 512.0 * sum_T + 32.0 * (double)max_windows * n_songs);
    float* ev = reinterpret_cast<float*>(const_cast<WaveEval*>(evs));
    VR_LAUNCH((istft_tile_kernel<false, const SongSeg, const WaveEval*, WindowSums>), dim3((unsigned)max_windows, n_songs), dim3(256), 0, st, pl, songs, 0, 0,
              (const float*)nullptr, 0, (const float*)nullptr, 0, 0, (const float*)nullptr, 0, ev, 0LL);
    VR_HIP(hipGetLastError());
}

// ---- spectrogram images: the launches -------------------------------------------------------------------------------
static int image_parts(long long max_pixels) {
    const long long chunks = (max_pixels + kImgChunk - 1) / kImgChunk;
    return (int)(chunks < kImgParts ? chunks : kImgParts);
}
static unsigned image_write_blocks(long long max_pixels) {
    const long long per = (long long)kImgChunk * kImgWriteChunks;
    return (unsigned)((max_pixels + per - 1) / per);
}

void launch_spec_image_many(const ImgSeg* jobs, int n, int channels, int bins, int max_T, double sum_T, bool cplx, int mode, hipStream_t st) {
    const long long max_pixels = (long long)bins * max_T;
    const SpecImage a{channels, mode, image_parts(max_pixels)};
    const double in_bytes = (double)channels * bins * sum_T * (cplx ? 8.0 : 4.0);
    const dim3 rg(a.nparts, n), wg(image_write_blocks(max_pixels), n);
    prof_note(0.0, in_bytes);
    if (cplx) VR_LAUNCH((mag_pad_kernel<true, const ImgSeg, false, SpecImage>), rg, dim3(256), 0, st, jobs, 0, (float*)nullptr, 0, 0, (unsigned long long*)nullptr, bins, (const float2*)nullptr, a);
    else VR_LAUNCH((mag_pad_kernel<false, const ImgSeg, false, SpecImage>), rg, dim3(256), 0, st, jobs, 0, (float*)nullptr, 0, 0, (unsigned long long*)nullptr, bins, (const float2*)nullptr, a);
    VR_HIP(hipGetLastError());
    prof_note(0.0, in_bytes + (channels == 2 ? 3.0 : 1.0) * bins * sum_T);
    if (cplx) VR_LAUNCH((apply_mask_kernel<true, const ImgSeg, SpecImage>), wg, dim3(256), 0, st, jobs, bins, 0, (const float*)nullptr, 0, (const float*)nullptr, 0, 0, (const float*)nullptr, (float2*)nullptr, (float2*)nullptr, a);
    else VR_LAUNCH((apply_mask_kernel<false, const ImgSeg, SpecImage>), wg, dim3(256), 0, st, jobs, bins, 0, (const float*)nullptr, 0, (const float*)nullptr, 0, 0, (const float*)nullptr, (float2*)nullptr, (float2*)nullptr, a);
    VR_HIP(hipGetLastError());
}

void launch_stem_image_many(const SongSeg* songs, const ImgSeg* jobs, int n_songs, int max_T, int bins, const float* mask, int W, int tta, bool cplx,
                            const float* wgt, double sum_T, hipStream_t st) {
    const long long max_pixels = (long long)bins * max_T;
    const StemImage a{jobs, image_parts(max_pixels)};
    // per pixel and channel: the spectrogram value and the mask (both passes of a TTA call); the write pass adds two 3-byte pixels
    const double in_bytes = 2.0 * bins * sum_T * (8.0 + (cplx ? 8.0 : 4.0) * (tta ? 2 : 1));
    const dim3 rg(a.nparts, n_songs), wg(image_write_blocks(max_pixels), n_songs);
    const float* mb = tta ? mask : nullptr;
    float* m = const_cast<float*>(mask);             // (mag_pad_kernel's slot is its output in the other forms; this one only reads it)
    const float2* w2 = reinterpret_cast<const float2*>(wgt);
    prof_note(0.0, in_bytes);
    if (cplx) VR_LAUNCH((mag_pad_kernel<true, const SongSeg, false, StemImage>), rg, dim3(256), 0, st, songs, 0, m, W, tta, (unsigned long long*)nullptr, bins, w2, a);
    else VR_LAUNCH((mag_pad_kernel<false, const SongSeg, false, StemImage>), rg, dim3(256), 0, st, songs, 0, m, W, tta, (unsigned long long*)nullptr, bins, w2, a);
    VR_HIP(hipGetLastError());
    prof_note(0.0, in_bytes + 6.0 * bins * sum_T);
    if (cplx) VR_LAUNCH((apply_mask_kernel<true, const SongSeg, StemImage>), wg, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, (float2*)nullptr, (float2*)nullptr, a);
    else VR_LAUNCH((apply_mask_kernel<false, const SongSeg, StemImage>), wg, dim3(256), 0, st, songs, bins, 0, mask, W, mb, W, 0, wgt, (float2*)nullptr, (float2*)nullptr, a);
    VR_HIP(hipGetLastError());
}

// vr_spec_image_many: n stored spectrograms -> n pictures.  No handle: one workspace for the call, the null stream.
void spec_image_many_api(int device, int n, const void* const* specs, bool on_dev, int channels, int bins, const int* T, bool cplx, int mode,
                         uint8_t* const* imgs, bool out_on_dev, float* ranges) {
    struct Buf { char* p = nullptr; ~Buf() { hipFree(p); } } buf;
    DeviceGuard dev_guard(device);
    const size_t el = cplx ? 8 : 4, pb = channels == 2 ? 3 : 1;
    std::vector<ImgSeg> tab((size_t)n);
    std::vector<char*> stage_in((size_t)n, nullptr), stage_out((size_t)n, nullptr);
    ImgSeg* tab_d = nullptr;
    float* range_d = nullptr;
    int max_T = 0;
    double sum_T = 0;
    for (int pass = 0; pass < 2; ++pass) {           // the same carve twice: once for the total, once for the pointers
        size_t off = 0;
        auto carve = [&](size_t bytes) { const size_t a = (off + 255) & ~size_t(255); off = a + bytes; return buf.p ? buf.p + a : nullptr; };
        tab_d = reinterpret_cast<ImgSeg*>(carve(sizeof(ImgSeg) * n));
        range_d = reinterpret_cast<float*>(carve(sizeof(float) * 2 * n));
        for (int i = 0; i < n; ++i) {
            const size_t pixels = (size_t)bins * T[i];
            ImgSeg& e = tab[i];
            e = ImgSeg{};
            e.T = T[i];
            stage_in[i] = on_dev ? nullptr : carve(pixels * channels * el);
            stage_out[i] = out_on_dev ? nullptr : carve(pixels * pb);
            e.src = on_dev ? specs[i] : stage_in[i];
            e.img[0] = out_on_dev ? imgs[i] : reinterpret_cast<uint8_t*>(stage_out[i]);
            e.part = reinterpret_cast<float4*>(carve(sizeof(float4) * kImgParts));
            e.range = range_d + 2 * i;
            if (!pass) { max_T = std::max(max_T, T[i]); sum_T += T[i]; }
        }
        if (pass) break;
        const size_t need = off + 256;
        if (hipMalloc(reinterpret_cast<void**>(&buf.p), need) != hipSuccess) {
            (void)hipGetLastError();
            buf.p = nullptr;
            throw Error(-4, "spec image: hipMalloc of " + std::to_string(need) + " bytes of workspace failed");
        }
    }
    hipStream_t st = nullptr;
    if (!on_dev)
        for (int i = 0; i < n; ++i)
            VR_HIP(hipMemcpyAsync(stage_in[i], specs[i], (size_t)bins * T[i] * channels * el, hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(tab_d, tab.data(), sizeof(ImgSeg) * n, hipMemcpyHostToDevice, st));
    launch_spec_image_many(tab_d, n, channels, bins, max_T, sum_T, cplx, mode, st);
    if (!out_on_dev)
        for (int i = 0; i < n; ++i)
            VR_HIP(hipMemcpyAsync(imgs[i], stage_out[i], (size_t)bins * T[i] * pb, hipMemcpyDeviceToHost, st));
    if (ranges) VR_HIP(hipMemcpyAsync(ranges, range_d, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
    VR_HIP(hipStreamSynchronize(st));
}

// ---- streaming separation (vr_stream_*): the STREAM instantiations -----------------------------------------------------------------
// Every launch covers what one step of the stream added: new frames, newly ready crops, newly final output segments.
bool stream_tiled_available(const FFTPlan& pl, int hop) { return tiled_signal_path(pl, hop); }

void launch_stft_stream(const FFTPlan& pl, const StreamSeg* seg, int n_seg, int new_frames, double new_samples, double sum_frames, hipStream_t st,
                        const PcmIn* pcm, double pcm_bytes) {
    const int M = pl.n_fft / 2, bins = M + 1;
    int F = tile_frames(pl, 0);
    if (F > 16) F = 16;
    F = F / TG * TG;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8;
    if (pcm) {                                           // the blocks of the entries are sample bytes (one PcmIn per entry)
        static std::atomic<unsigned long long> attr_pcm{0};
        ensure_lds_attr(attr_pcm, reinterpret_cast<const void*>(stft_tile_kernel<const StreamSeg, const PcmIn*>), 160 * 1024);
        prof_note(0.0, pcm_bytes + 2.0 * 8.0 * (double)bins * sum_frames);
        const int blocks = new_frames > 0 ? (new_frames + F - 1) / F : 1;
        VR_LAUNCH((stft_tile_kernel<const StreamSeg, const PcmIn*>), dim3((unsigned)blocks, 2, (unsigned)n_seg), dim3(1024), lds, st, pl, seg, 0LL, 0, F,
                  nullptr, pcm);
        VR_HIP(hipGetLastError());
        return;
    }
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(stft_tile_kernel<const StreamSeg>), 160 * 1024);
    prof_note(0.0, 2.0 * (4.0 * new_samples + 8.0 * (double)bins * sum_frames));
    // (a step without a new frame still launches one workgroup per channel: it moves the input tail on)
    const int blocks = new_frames > 0 ? (new_frames + F - 1) / F : 1;
    VR_LAUNCH((stft_tile_kernel<const StreamSeg>), dim3((unsigned)blocks, 2, (unsigned)n_seg), dim3(1024), lds, st, pl, seg, 0LL, 0, F, nullptr);
    VR_HIP(hipGetLastError());
}

void launch_stream_stats(const StreamSeg* seg, int bins, int new_frames, unsigned long long* part, hipStream_t st) {
    prof_note(0.0, 2.0 * (double)bins * 8.0 * new_frames);
    VR_LAUNCH((mag_pad_kernel<false, const StreamSeg>), dim3(2 * bins), dim3(256), 0, st, seg, 0, nullptr, 0, 0, part, bins, nullptr);
    VR_HIP(hipGetLastError());
}

void launch_stream_gather(const StreamSeg* seg, const int2* crops, int count, bool cplx, int bins, int max_bin, int cropsize, float* dst,
                          hipStream_t st) {
    prof_note(0.0, (double)count * 2 * max_bin * cropsize * (8.0 + (cplx ? 8.0 : 4.0)));
    unsigned long long* list = reinterpret_cast<unsigned long long*>(const_cast<int2*>(crops));
    if (cplx) VR_LAUNCH((mag_pad_kernel<true, const StreamSeg, true>), dim3(2 * max_bin, count), dim3(256), 0, st, seg, cropsize, dst, max_bin, 0, list, bins, nullptr);
    else VR_LAUNCH((mag_pad_kernel<false, const StreamSeg, true>), dim3(2 * max_bin, count), dim3(256), 0, st, seg, cropsize, dst, max_bin, 0, list, bins, nullptr);
    VR_HIP(hipGetLastError());
}

void launch_istft_stream(const FFTPlan& pl, const StreamSeg* seg, int n_seg, int segments, double sum_segments, bool cplx, bool tta, int which,
                         hipStream_t st, bool pcm16) {
    const int M = pl.n_fft / 2, bins = M + 1;
    if (segments < 1) return;
    const int F = tile_frames(pl, M);
    const int S = F - 1;
    const size_t lds = (size_t)TG * M * 8 + (size_t)bins * F * 8 + (size_t)M * 4;
    const dim3 grid((unsigned)((segments + S - 1) / S), 2, (unsigned)n_seg);
    prof_note(0.0, 2.0 * ((double)bins * sum_segments * (8.0 + (cplx ? 8.0 : 4.0) * (tta ? 2 : 1)) + (pcm16 ? 2.0 : 4.0) * (double)M * sum_segments));
    if (pcm16) {                                         // y_wave / v_wave of the entries point to interleaved int16
        if (cplx) {
            static std::atomic<unsigned long long> attr_done{0};
            ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<true, const StreamSeg, WavePcm16Out>), 160 * 1024);
            VR_LAUNCH((istft_tile_kernel<true, const StreamSeg, WavePcm16Out>), grid, dim3(1024), lds, st, pl, seg, 0, S, nullptr, 0, nullptr, 0, 0, nullptr, which, nullptr, 0LL);
        } else {
            static std::atomic<unsigned long long> attr_done{0};
            ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<false, const StreamSeg, WavePcm16Out>), 160 * 1024);
            VR_LAUNCH((istft_tile_kernel<false, const StreamSeg, WavePcm16Out>), grid, dim3(1024), lds, st, pl, seg, 0, S, nullptr, 0, nullptr, 0, 0, nullptr, which, nullptr, 0LL);
        }
        VR_HIP(hipGetLastError());
        return;
    }
    if (cplx) {
        static std::atomic<unsigned long long> attr_done{0};
        ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<true, const StreamSeg>), 160 * 1024);
        VR_LAUNCH((istft_tile_kernel<true, const StreamSeg>), grid, dim3(1024), lds, st, pl, seg, 0, S, nullptr, 0, nullptr, 0, 0, nullptr, which, nullptr, 0LL);
    } else {
        static std::atomic<unsigned long long> attr_done{0};
        ensure_lds_attr(attr_done, reinterpret_cast<const void*>(istft_tile_kernel<false, const StreamSeg>), 160 * 1024);
        VR_LAUNCH((istft_tile_kernel<false, const StreamSeg>), grid, dim3(1024), lds, st, pl, seg, 0, S, nullptr, 0, nullptr, 0, 0, nullptr, which, nullptr, 0LL);
    }
    VR_HIP(hipGetLastError());
}

void launch_stream_post(const StreamSeg* seg, int n_seg, int post_frames, double sum_frames, bool walk, bool cplx, bool tta, int bins,
                        hipStream_t st) {
    if (post_frames > 0) {
        const dim3 grid((unsigned)((post_frames + kStreamMinFrames - 1) / kStreamMinFrames), (unsigned)n_seg);
        prof_note(0.0, 2.0 * (double)bins * sum_frames * (cplx ? 8.0 : 4.0) * (tta ? 2 : 1));
        if (cplx) VR_LAUNCH((frame_min_kernel<true, const StreamSeg>), grid, dim3(256), 0, st, 2 * bins, 0, nullptr, 0, nullptr, 0, 0, seg);
        else VR_LAUNCH((frame_min_kernel<false, const StreamSeg>), grid, dim3(256), 0, st, 2 * bins, 0, nullptr, 0, nullptr, 0, 0, seg);
        VR_HIP(hipGetLastError());
    }
    if (walk) {
        prof_note(0.0, 8.0 * sum_frames);
        if (cplx) VR_LAUNCH((frame_min_kernel<true, const StreamSeg>), dim3(1, (unsigned)n_seg), dim3(256), 0, st, 0, 0, nullptr, 0, nullptr, 0, 0, seg);
        else VR_LAUNCH((frame_min_kernel<false, const StreamSeg>), dim3(1, (unsigned)n_seg), dim3(256), 0, st, 0, 0, nullptr, 0, nullptr, 0, 0, seg);
        VR_HIP(hipGetLastError());
    }
}

}  // namespace vr
