// Training input pipeline on the device: everything VocalRemoverTrainingSet.__getitem__
// (lib/dataset.py:105-120) does AFTER the random decisions and the file reads --
//   X /= coef, y /= coef                                   (dataset.py:108-110)
//   aggressively_remove_vocal                               (dataset.py:48-56)
//   channel swap / inst-only                                (dataset.py:68-83)
//   mixup with a second, independently augmented crop       (dataset.py:85-103)
//   np.abs, and the [T,2,bins] -> [2,bins,T] transpose      (dataset.py:63-64,116-117)
//   (or, for a complex-mask model, the complex values themselves: dataset.py:120, the commented `return X, y`)
// -- as ONE HBM-bound kernel over a whole batch.  The host keeps what is inherently host work: drawing
// the numpy random numbers in the reference's order and seek-reading cropsize rows of the cached .npy.
#include <type_traits>

#include "kernels.h"

namespace vr {

__device__ __forceinline__ float2 cdivf(float2 a, float c) { return make_float2(a.x / c, a.y / c); }

// One (frame t, channel c, bin) element of one crop after /coef and the per-sample augmentations.
__device__ __forceinline__ void aug_element(const float2* __restrict__ X, const float2* __restrict__ Y, long long base, int bins,
                                            int t, int c, int bin, float coef, int reduce, int swap, int inst, float rw,
                                            float2& xo, float2& yo) {
    const int cs = swap ? 1 - c : c;
    const long long i = base + ((long long)t * 2 + cs) * bins + bin;
    float2 x = cdivf(X[i], coef), y = cdivf(Y[i], coef);
    if (reduce) {
        const float xm = hypotf(x.x, x.y), ym = hypotf(y.x, y.y);
        float v = xm - ym;
        v = v > ym ? v : 0.f;
        const float ym2 = fmaxf(ym - v * rw, 0.f);
        const float ux = ym > 0.f ? y.x / ym : 1.f, uy = ym > 0.f ? y.y / ym : 0.f;      // exp(1j * angle(y))
        y = make_float2(ym2 * ux, ym2 * uy);
    }
    if (inst) x = y;
    xo = x;
    yo = y;
}

// a = 0.5f * (a + o): the mono augmentation of one element from its two channels (lib/dataset.py:81-83, X.mean(axis=0))
__device__ __forceinline__ void aug_mono(float2& a, float2 o) {
    a = make_float2(__fmul_rn(0.5f, __fadd_rn(a.x, o.x)), __fmul_rn(0.5f, __fadd_rn(a.y, o.y)));
}

// grid: (ceil(T/32), ceil(bins/32), B*2); block (32, 8).  32x32 tile transposed through LDS so that both the
// reads (bin-contiguous) and the writes (frame-contiguous) are coalesced.
// Two forms, which differ only in where the four crops of sample b lie.  Dense (vr_augment_batch): X, Y, Xi, Yi are staged batches,
// sample b at b * T * 2 * bins of each.  Resident (vr_dataset_batch): the first argument is a table with one AugCrops per sample,
// every pointer already advanced to the sample's start row inside the [rows][2][bins] slab of its song (the mixup pair repeats the
// first two when the sample has no partner); the other three pointer arguments are unused.
// kComplex (training a complex-mask model): everything before the final np.abs is the same; the augmented x, y themselves are stored,
// complex64 [B][2][bins][T].  The real and imaginary parts cross the transpose in tiles of their own (four float tiles of 33-word rows,
// the bank-conflict-free layout of the magnitude form; a float2 tile would put a 64-bit read at a 66-word stride).
// DESC = AugDescEx (the _ex entry points): three more branches, each behind `if constexpr (kEx)`, so the AugDesc
// instantiations compile from the statements they always had.  d.flags is uniform over the block: none of them diverges.
//   mono    the element of the other channel is read as well and both blocks of the sample store 0.5f * (L + R); L + R is R + L in
//           IEEE arithmetic, so the two channels of the output hold the same bits.  Only a sample (or partner) with the bit reads twice.
//   remix   the partner's crop with its own coef and swap bit, no reduce and no inst-only: v = X_j - y_j, y = g_y y, X = y + g_v v.
//           One rounding per operation, spelled with the _rn intrinsics, so no instantiation may contract them differently.
template <bool kResident, bool kComplex, class DESC = AugDesc>
__global__ __launch_bounds__(256) void augment_kernel(std::conditional_t<kResident, const AugCrops*, const float2*> __restrict__ X,
                                                      const float2* __restrict__ Y, const float2* __restrict__ Xi,
                                                      const float2* __restrict__ Yi, const DESC* __restrict__ desc,
                                                      const float* __restrict__ rw, int T, int bins, float* __restrict__ Xmag,
                                                      float* __restrict__ Ymag) {
    constexpr int NT = kComplex ? 2 : 1;
    __shared__ float tx[NT][32][33], ty[NT][32][33];
    const int b = blockIdx.z >> 1, c = blockIdx.z & 1;
    const int t0 = blockIdx.x * 32, bin0 = blockIdx.y * 32;
    constexpr bool kEx = std::is_same<DESC, AugDescEx>::value;
    static_assert(kEx || std::is_same<DESC, AugDesc>::value, "augment_kernel: unknown descriptor");
    const DESC d = desc[b];
    const float2* __restrict__ Xc;
    long long base;
    if constexpr (kResident) {
        const AugCrops s = X[b];                   // (b is uniform over the block: scalar loads)
        Xc = s.X; Y = s.y; Xi = s.X_mix; Yi = s.y_mix;
        base = 0;
    } else {
        Xc = X;
        base = (long long)b * T * 2 * bins;
    }
    const int bin = bin0 + threadIdx.x;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int t = t0 + r;
        float2 x = make_float2(0.f, 0.f), y = make_float2(0.f, 0.f);
        if (t < T && bin < bins) {
            const float w = rw ? rw[bin] : 0.f;
            aug_element(Xc, Y, base, bins, t, c, bin, d.coef, d.flags & 1, d.flags & 2, d.flags & 4, w, x, y);
            if constexpr (kEx) {
                if (d.flags & kAugMono) {
                    float2 xo, yo;
                    aug_element(Xc, Y, base, bins, t, 1 - c, bin, d.coef, d.flags & 1, d.flags & 2, d.flags & 4, w, xo, yo);
                    aug_mono(x, xo);
                    aug_mono(y, yo);
                }
                if (d.flags & kAugRemix) {
                    float2 xj, yj;
                    aug_element(Xi, Yi, base, bins, t, c, bin, d.coef_mix, 0, d.flags & 32, 0, w, xj, yj);
                    y = make_float2(__fmul_rn(d.gain_y, y.x), __fmul_rn(d.gain_y, y.y));
                    x = make_float2(__fadd_rn(y.x, __fmul_rn(d.gain_v, __fsub_rn(xj.x, yj.x))),
                                    __fadd_rn(y.y, __fmul_rn(d.gain_v, __fsub_rn(xj.y, yj.y))));
                }
            }
            if (d.flags & 8) {
                float2 xi, yi;
                aug_element(Xi, Yi, base, bins, t, c, bin, d.coef_mix, d.flags & 16, d.flags & 32, d.flags & 64, w, xi, yi);
                if constexpr (kEx) {
                    if (d.flags & kAugMixMono) {
                        float2 xo, yo;
                        aug_element(Xi, Yi, base, bins, t, 1 - c, bin, d.coef_mix, d.flags & 16, d.flags & 32, d.flags & 64, w, xo, yo);
                        aug_mono(xi, xo);
                        aug_mono(yi, yo);
                    }
                }
                const float l = d.lam, m = 1.f - d.lam;
                x = make_float2(l * x.x + m * xi.x, l * x.y + m * xi.y);
                y = make_float2(l * y.x + m * yi.x, l * y.y + m * yi.y);
            }
        }
        if constexpr (kComplex) {
            tx[0][r][threadIdx.x] = x.x; tx[1][r][threadIdx.x] = x.y;
            ty[0][r][threadIdx.x] = y.x; ty[1][r][threadIdx.x] = y.y;
        } else {
            tx[0][r][threadIdx.x] = hypotf(x.x, x.y);
            ty[0][r][threadIdx.x] = hypotf(y.x, y.y);
        }
    }
    __syncthreads();
    const int t = t0 + threadIdx.x;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int bo = bin0 + r;
        if (t < T && bo < bins) {
            const long long o = (((long long)b * 2 + c) * bins + bo) * T + t;
            if constexpr (kComplex) {
                reinterpret_cast<float2*>(Xmag)[o] = make_float2(tx[0][threadIdx.x][r], tx[1][threadIdx.x][r]);
                reinterpret_cast<float2*>(Ymag)[o] = make_float2(ty[0][threadIdx.x][r], ty[1][threadIdx.x][r]);
            } else {
                Xmag[o] = tx[0][threadIdx.x][r];
                Ymag[o] = ty[0][threadIdx.x][r];
            }
        }
    }
}

// ---- pitch-shifted training pairs (vr_pitch_*): the offline augmentation of the reference's augment.py --------
// Two more forms under the family's name, selected by the argument struct the kernel is instantiated with (kernels.h).
//
// PitchDiff: v = mix - inst over n samples, one float32 subtraction each (the vocals wave the pair entry shifts beside the instrumental).
//
// PitchVocoder: librosa.phase_vocoder on `signals` spectrograms [bins][T] -> [bins][Tout], Tout = ceil(T / rate).  Output frame t reads
// the input at s = t * rate (double): i = int(s), a = s - i, mag = (1 - a) |D[i]| + a |D[i + 1]|, and its phase is
//     acc[t] = angle(D[0]) + sum over u < t of (phi + wrap(angle(D[i_u + 1]) - angle(D[i_u]) - phi)),   phi = pi hop k / (bins - 1),
// an exclusive prefix sum along time.  Everything up to the store is fp64 (a float32 phase is off by 1e-2 of the wave's peak after a
// few hundred frames): angles by atan2 of the complex64 parts, the sum, the magnitude, sincos; the product mag * (cos, sin) is rounded
// to float once.  A wave owns one (signal, bin) row; its lanes run along t, 64 frames per step: a shuffle scan inside the wave, the
// total carried to the next step in a double.  No LDS, no barrier, no atomics: the order of the additions is fixed, so two calls agree
// bit for bit.  Columns at and past T read as zero, as the two zero columns librosa appends.
// grid (ceil(bins / 4), signals), block 256 = four rows.
template <class FORM>
__global__ __launch_bounds__(256) void augment_kernel(FORM a) {
    if constexpr (std::is_same<FORM, PitchDiff>::value) {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if (i < a.n) a.v[i] = a.mix[i] - a.inst[i];
    } else {
        static_assert(std::is_same<FORM, PitchVocoder>::value, "augment_kernel: unknown form");
        const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (k >= a.bins) return;                                    // (a whole wave leaves: nothing below is workgroup-wide)
        const long long r = (long long)blockIdx.y * a.bins + k;
        const float2* __restrict__ row = a.D + r * a.T;
        float2* __restrict__ orow = a.out + r * a.Tout;
        const double PI = 3.14159265358979323846, TWO_PI = 2.0 * PI;
        // np.linspace(0, pi * hop, bins)[k]: k * step, the last one the end point itself
        const double phi = k == a.bins - 1 ? PI * (double)a.hop : (double)k * ((PI * (double)a.hop) / (double)(a.bins - 1));
        const float2 first = row[0];
        double carry = atan2((double)first.y, (double)first.x);
        for (int t0 = 0; t0 < a.Tout; t0 += 64) {
            const int t = t0 + lane;
            double inc = 0.0, mag = 0.0;
            if (t < a.Tout) {
                const double s = (double)t * a.rate;
                const int i = (int)s;
                const double al = s - (double)i;
                const float2 c0 = i < a.T ? row[i] : make_float2(0.f, 0.f);
                const float2 c1 = i + 1 < a.T ? row[i + 1] : make_float2(0.f, 0.f);
                const double x0 = c0.x, y0 = c0.y, x1 = c1.x, y1 = c1.y;
                mag = (1.0 - al) * sqrt(x0 * x0 + y0 * y0) + al * sqrt(x1 * x1 + y1 * y1);
                double d = atan2(y1, x1) - atan2(y0, x0) - phi;
                d = d - TWO_PI * rint(d / TWO_PI);
                inc = phi + d;
            }
            double incl = inc;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const double up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            double excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 0.0;
            const double acc = carry + excl;
            carry += __shfl(incl, 63, 64);
            if (t < a.Tout) {
                double sn, cs;
                sincos(acc, &sn, &cs);
                orow[t] = make_float2((float)(mag * cs), (float)(mag * sn));
            }
        }
    }
}

// ---- the resident song store's own forms (vr_dataset_windows, vr_dataset_peak) ----------------------------------
// A third template under the family's name, again selected by the argument struct; the six instantiations above are not touched.
//
// SongWindows (kFlag: complex64 output): the resident form of the first kernel -- same grid, same 32 x 32 tile through LDS rows of 33
// words -- without augmentation and with the window free to leave its song: the per-sample entry carries the song's rows and a signed
// start, a row outside [0, rows) reads as zero, and every value read is multiplied by the entry's scale (one float32 product per part:
// 1 / peak of the song, numpy's complex64 / float32).
//
// SongPeak (kFlag: the second of its two launches): the element of largest np.abs of one song's two slabs.  The key is np.abs itself,
// the float32 numpy computes for a complex64 (numpy_cabsf, kernels.h: five IEEE operations, so the device's value is numpy's), and the
// candidate is the key and its position in the [X | y] sequence of complex elements; a larger key wins, an equal key at a lower
// position wins, so the result does not depend on the grid.  A NaN key sets a flag carried beside the candidate.  First launch:
// workgroup g takes float4 1024 g + 256 k + lane of the sequence (k < 4: four independent 16-byte loads a lane, two complex64 each),
// strides by the grid, reduces across the wave by shuffles and across its four waves through LDS, and stores one partial.  Second
// launch: one workgroup over the partials; it reads the winning element back and stores candidate and element for the host.  No atomics.
__device__ __forceinline__ void peak_take(float& k, unsigned long long& p, float ok, unsigned long long op) {
    if (ok > k || (ok == k && op < p)) { k = ok; p = op; }
}

__device__ __forceinline__ void peak_element(float re, float im, unsigned long long pos, float& k, unsigned long long& p, unsigned& bad) {
    const float key = numpy_cabsf(re, im);
    bad |= key != key ? 1u : 0u;
    if (key > k) { k = key; p = pos; }               // (a lane meets its positions in rising order: the first of equals stays)
}

// -> thread 0 of the workgroup holds the workgroup's candidate and flag
__device__ __forceinline__ void peak_reduce(float& k, unsigned long long& p, unsigned& bad) {
    __shared__ float sk[4];
    __shared__ unsigned long long sp[4];
    __shared__ unsigned sb[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ok = __shfl_down(k, off, 64);
        const unsigned long long op = __shfl_down(p, off, 64);
        bad |= __shfl_down(bad, off, 64);
        peak_take(k, p, ok, op);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[wave] = k; sp[wave] = p; sb[wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) { peak_take(k, p, sk[w], sp[w]); bad |= sb[w]; }
}

template <class FORM, bool kFlag>
__global__ __launch_bounds__(256) void augment_kernel(FORM a) {
    if constexpr (std::is_same<FORM, SongWindows>::value) {
        constexpr int NT = kFlag ? 2 : 1;
        __shared__ float tx[NT][32][33], ty[NT][32][33];
        const int b = blockIdx.z >> 1, c = blockIdx.z & 1;
        const int t0 = blockIdx.x * 32, bin0 = blockIdx.y * 32;
        const int T = a.T, bins = a.bins;
        const SongWindow s = a.table[b];                   // (b is uniform over the block: scalar loads)
        const int bin = bin0 + threadIdx.x;
        for (int r = threadIdx.y; r < 32; r += 8) {
            const int t = t0 + r;
            float2 x = make_float2(0.f, 0.f), y = make_float2(0.f, 0.f);
            if (t < T && bin < bins) {
                const long long row = s.start + t;         // (start + T does not overflow: checked by the host)
                if (row >= 0 && row < s.rows) {
                    const long long i = (row * 2 + c) * bins + bin;
                    const float2 xv = s.X[i], yv = s.y[i];
                    x = make_float2(xv.x * s.scale, xv.y * s.scale);
                    y = make_float2(yv.x * s.scale, yv.y * s.scale);
                }
            }
            if constexpr (kFlag) {
                tx[0][r][threadIdx.x] = x.x; tx[1][r][threadIdx.x] = x.y;
                ty[0][r][threadIdx.x] = y.x; ty[1][r][threadIdx.x] = y.y;
            } else {
                tx[0][r][threadIdx.x] = hypotf(x.x, x.y);
                ty[0][r][threadIdx.x] = hypotf(y.x, y.y);
            }
        }
        __syncthreads();
        const int t = t0 + threadIdx.x;
        for (int r = threadIdx.y; r < 32; r += 8) {
            const int bo = bin0 + r;
            if (t < T && bo < bins) {
                const long long o = (((long long)b * 2 + c) * bins + bo) * T + t;
                if constexpr (kFlag) {
                    reinterpret_cast<float2*>(a.X_out)[o] = make_float2(tx[0][threadIdx.x][r], tx[1][threadIdx.x][r]);
                    reinterpret_cast<float2*>(a.y_out)[o] = make_float2(ty[0][threadIdx.x][r], ty[1][threadIdx.x][r]);
                } else {
                    a.X_out[o] = tx[0][threadIdx.x][r];
                    a.y_out[o] = ty[0][threadIdx.x][r];
                }
            }
        }
    } else {
        static_assert(std::is_same<FORM, SongPeak>::value, "augment_kernel: unknown form");
        float k = -1.f;
        unsigned long long p = ~0ull;
        unsigned bad = 0;
        if constexpr (!kFlag) {
            const long long half = a.n >> 1, total = 2 * half;        // float4s of one slab, of both
            const float4* __restrict__ X4 = reinterpret_cast<const float4*>(a.X);
            const float4* __restrict__ Y4 = reinterpret_cast<const float4*>(a.y);
            for (long long base = (long long)blockIdx.x * 1024; base < total; base += (long long)gridDim.x * 1024) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long q = base + u * 256 + threadIdx.x;
                    v[u] = q >= total ? make_float4(0.f, 0.f, 0.f, 0.f) : q < half ? X4[q] : Y4[q - half];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long q = base + u * 256 + threadIdx.x;
                    if (q < total) {
                        peak_element(v[u].x, v[u].y, 2ull * (unsigned long long)q, k, p, bad);
                        peak_element(v[u].z, v[u].w, 2ull * (unsigned long long)q + 1, k, p, bad);
                    }
                }
            }
            peak_reduce(k, p, bad);
            if (threadIdx.x == 0) a.part[blockIdx.x] = PeakCand{p, k, bad, 0.f, 0.f};
        } else {
            for (int i = threadIdx.x; i < a.parts; i += 256) {
                const PeakCand c = a.part[i];
                peak_take(k, p, c.key, c.pos);
                bad |= c.bad;
            }
            peak_reduce(k, p, bad);
            if (threadIdx.x == 0) {
                float2 e = make_float2(0.f, 0.f);                    // (every element NaN: no candidate, the flag says so)
                if (p < 2ull * (unsigned long long)a.n) e = p < (unsigned long long)a.n ? a.X[p] : a.y[p - (unsigned long long)a.n];
                a.part[a.parts] = PeakCand{p, k, bad, e.x, e.y};
            }
        }
    }
}

int song_peak_parts(long long n) {
    const long long groups = (n + 1023) / 1024;         // n complex64 of each slab = n float4 in all, 1024 a workgroup and step
    return (int)(groups < kPeakParts ? groups : kPeakParts);
}

void launch_song_peak(const float2* X, const float2* y, long long n, PeakCand* ws, hipStream_t st) {
    const int parts = song_peak_parts(n);
    const SongPeak a{X, y, n, ws, parts};
    prof_note(0.0, 16.0 * (double)n);
    VR_LAUNCH((augment_kernel<SongPeak, false>), dim3((unsigned)parts), dim3(256), 0, st, a);
    VR_HIP(hipGetLastError());
    VR_LAUNCH((augment_kernel<SongPeak, true>), dim3(1), dim3(256), 0, st, a);
    VR_HIP(hipGetLastError());
}

void launch_song_windows(const SongWindow* table, int B, int T, int bins, float* X_out, float* y_out, bool out_complex, hipStream_t st) {
    const dim3 grid((T + 31) / 32, (bins + 31) / 32, B * 2), block(32, 8);
    const SongWindows a{table, T, bins, X_out, y_out};
    if (out_complex) VR_LAUNCH((augment_kernel<SongWindows, true>), grid, block, 0, st, a);
    else VR_LAUNCH((augment_kernel<SongWindows, false>), grid, block, 0, st, a);
    VR_HIP(hipGetLastError());
}

void launch_pitch_diff(const float* mix, const float* inst, float* v, long long n, hipStream_t st) {
    if (n <= 0) return;
    prof_note(0.0, 12.0 * (double)n);
    VR_LAUNCH(augment_kernel<PitchDiff>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, PitchDiff{mix, inst, v, n});
    VR_HIP(hipGetLastError());
}

void launch_phase_vocoder(const float2* D, float2* out, int signals, int bins, int T, int Tout, int hop, double rate, hipStream_t st) {
    prof_note(0.0, 8.0 * (double)signals * bins * ((double)T + (double)Tout));      // each spectrogram read once, the stretched one written
    VR_LAUNCH(augment_kernel<PitchVocoder>, dim3((unsigned)((bins + 3) / 4), (unsigned)signals), dim3(256), 0, st,
              PitchVocoder{D, out, bins, T, Tout, hop, rate});
    VR_HIP(hipGetLastError());
}

void launch_augment(const float2* X, const float2* Y, const float2* Xi, const float2* Yi, const AugDesc* desc, const float* rw,
                    int B, int T, int bins, float* Xmag, float* Ymag, bool out_complex, hipStream_t st) {
    const dim3 grid((T + 31) / 32, (bins + 31) / 32, B * 2), block(32, 8);
    if (out_complex) VR_LAUNCH((augment_kernel<false, true>), grid, block, 0, st, X, Y, Xi, Yi, desc, rw, T, bins, Xmag, Ymag);
    else VR_LAUNCH((augment_kernel<false, false>), grid, block, 0, st, X, Y, Xi, Yi, desc, rw, T, bins, Xmag, Ymag);
    VR_HIP(hipGetLastError());
}

void launch_augment_resident(const AugCrops* table, const AugDesc* desc, const float* rw, int B, int T, int bins, float* Xmag,
                             float* Ymag, bool out_complex, hipStream_t st) {
    const dim3 grid((T + 31) / 32, (bins + 31) / 32, B * 2), block(32, 8);
    const float2* const unused = nullptr;
    if (out_complex) VR_LAUNCH((augment_kernel<true, true>), grid, block, 0, st, table, unused, unused, unused, desc, rw, T, bins, Xmag, Ymag);
    else VR_LAUNCH((augment_kernel<true, false>), grid, block, 0, st, table, unused, unused, unused, desc, rw, T, bins, Xmag, Ymag);
    VR_HIP(hipGetLastError());
}

void launch_augment(const float2* X, const float2* Y, const float2* Xi, const float2* Yi, const AugDescEx* desc, const float* rw,
                    int B, int T, int bins, float* Xmag, float* Ymag, bool out_complex, hipStream_t st) {
    const dim3 grid((T + 31) / 32, (bins + 31) / 32, B * 2), block(32, 8);
    if (out_complex) VR_LAUNCH((augment_kernel<false, true, AugDescEx>), grid, block, 0, st, X, Y, Xi, Yi, desc, rw, T, bins, Xmag, Ymag);
    else VR_LAUNCH((augment_kernel<false, false, AugDescEx>), grid, block, 0, st, X, Y, Xi, Yi, desc, rw, T, bins, Xmag, Ymag);
    VR_HIP(hipGetLastError());
}

void launch_augment_resident(const AugCrops* table, const AugDescEx* desc, const float* rw, int B, int T, int bins, float* Xmag,
                             float* Ymag, bool out_complex, hipStream_t st) {
    const dim3 grid((T + 31) / 32, (bins + 31) / 32, B * 2), block(32, 8);
    const float2* const unused = nullptr;
    if (out_complex) VR_LAUNCH((augment_kernel<true, true, AugDescEx>), grid, block, 0, st, table, unused, unused, unused, desc, rw, T, bins, Xmag, Ymag);
    else VR_LAUNCH((augment_kernel<true, false, AugDescEx>), grid, block, 0, st, table, unused, unused, unused, desc, rw, T, bins, Xmag, Ymag);
    VR_HIP(hipGetLastError());
}

}  // namespace vr
