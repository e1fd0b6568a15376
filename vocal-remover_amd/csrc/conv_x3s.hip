// Direct 3x3 STRIDE-2 convolution on the fp16 matrix pipe: conv_x3h.hip's schedule and arithmetic (fp32-grade products from three fp16
// products, per-chunk power-of-two pixel scaling with a running shift, weights by LDS-DMA, pixel registers loaded two chunks ahead
// with hand-placed waits, 14 matrix-instruction groups per 8-channel chunk), with the stride taken in the LOADER.  mfma_mode 3, eval:
// the encoder's enc2..enc5.conv1 layers with at least 32 output columns and more than 16 input channels (x3s_pick).
//
// The B operand of v_mfma_f32_32x32x16_f16 wants the 32 output pixels of a row side by side.  At stride 2 these are every second
// column of the halo tile, so the two fp16 planes keep every halo row SPLIT BY COLUMN PARITY:
//   halo tile = (2 TH + 1) rows x 66 columns, input rows 2 h0 - 1 ..., input columns 2 w0 - 2 ... 2 w0 + 63
//   row r of a plane:  E run, 33 entries: input columns 2 w0 - 1 + 2 u (odd)  |  O run, 33 entries: input columns 2 w0 - 2 + 2 u (even)
//   output pixel (r, j), tap (ty, tx) reads halo row 2 r + ty and  tx = 0: E[j]   tx = 1: O[j + 1]   tx = 2: E[j + 1]
// so every operand read stays 16 contiguous bytes per lane at a compile-time offset, as in conv_x3h, and the multiply phase is
// the stride-1 kernel's for the same Cin, Cout and OUTPUT size (Cin / 8 chunks of 14 groups; the space-to-depth form had four
// times the chunks and 24 groups per 8 real channels).  Only the pixel side grows: 17 x 66 input pixels per 8 x 32 outputs.
//
// Pixels are loaded as (even, odd) column PAIRS with buffer_load_dwordx2: pair u of a row = columns 2 w0 - 2 + 2 u and + 1, which
// land at the same index u of the O and the E run.  17 x 33 = 561 pair slots are 3 passes of 256 threads, 24 loads per chunk:
// two chunks in flight + the weight DMAs stay below the 6 bits of vmcnt (2 * 24 + 4 = 52), where single-column loads (1105 slots,
// 40 loads per chunk) would not.  A pair never straddles the image edge when Win is even, and is 8-byte aligned when the pitches
// are even too: x3s_pick asks for both, anything else keeps the fp32 kernel.  (O[0], column 2 w0 - 2, is loaded and split but
// never multiplied; it takes part in the chunk maximum -- one more column in "the largest pixel of the tile's chunk".)
//
// One plain source (no pending affine, no post, no upsample, slope 1): what the network feeds these layers in eval.
#include <type_traits>

#include "conv_epilogue.h"
#include "conv_stage.h"
#include "kernels.h"
#include "lds_dma.h"
#include "x3h_common.h"

namespace vr {

typedef float vr_f32x2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ vr_f32x2s x3s_load2(i32x4 rsrc, int voff) {
    vr_f32x2s v;
    asm volatile("buffer_load_dwordx2 %0, %1, %2, 0 offen" : "=v"(v) : "v"(voff), "s"(rsrc) : "memory");
    return v;
}
// s_waitcnt vmcnt(N) that the uses of the eight register pairs cannot be scheduled across (x3h_wait8 for pairs; the comment names
// them for tools/asm_inflight_audit2.py)
template <int N>
__device__ __forceinline__ void x3s_wait8(vr_f32x2s (&r)[8]) {
    asm volatile("s_waitcnt vmcnt(%8) ; landed %0 %1 %2 %3 %4 %5 %6 %7"
                 : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])
                 : "n"(N) : "memory");
}

template <int MT, int TH>
struct X3sCfg {
    static constexpr int TW = 32, CK = 8, KK = 9;
    static constexpr int ROWS = 2 * TH + 1, RUN = TW + 1, RP = 2 * RUN;   // halo rows; entries of a parity run; entries of a plane row
    static constexpr int NSLOT = ROWS * RUN;                     // column pairs a workgroup loads per channel
    static constexpr int NPASS = (NSLOT + 255) / 256;
    static constexpr int WM = MT / 32, WN = TH / 4;
    static constexpr int PLANE = ROWS * RP * 16;                 // bytes of one fp16 plane (8 channels per pixel)
    static constexpr int P_BYTES = 2 * PLANE;
    static constexpr int NWP = KK * 2 * MT;                      // 16-byte weight operands per chunk
    static constexpr int W_BYTES = NWP * 16;
    static constexpr int NWPASS = (NWP + 255) / 256;
    static constexpr int E_OFF = P_BYTES + 2 * W_BYTES;          // epilogue constants of the cout tile: bias, scale, shift, 1 / weight scale [4][MT] fp32
    static constexpr int M_OFF = E_OFF + 4 * MT * 4;             // the four wave maxima of the chunk being split (uint bits of |x|)
    static constexpr int LDS_BYTES = M_OFF + 16;
    // vector-memory operations a wave issues per chunk: 8 * NPASS pixel loads (always, also beyond Cin: empty descriptor), and at
    // least NWMIN weight DMAs
    static constexpr int NXL = 8 * NPASS, NWMIN = (NWP / 64) / 4;
    static constexpr int NG = 14;                                // matrix-instruction groups per chunk: X0 X1 Y01 X2 X3 Y23 ... X8 Y8
    // entry of tap column tx inside a plane row, for output column 0
    static constexpr int ex(int tx) { return tx == 0 ? 0 : (tx == 1 ? RUN + 1 : 1); }
    static_assert(TH % 4 == 0 && MT % 32 == 0 && 2 * LDS_BYTES <= 160 * 1024 && 2 * NXL + NWMIN < 64, "tile");
};

template <int MT, int TH>
__global__ __launch_bounds__(256, 2) void conv_x3h_kernel_s2(const ConvArgs a) {
    using Cfg = X3sCfg<MT, TH>;
    constexpr int TW = Cfg::TW, KK = Cfg::KK, RP = Cfg::RP, RUN = Cfg::RUN, NSLOT = Cfg::NSLOT, NPASS = Cfg::NPASS, WM = Cfg::WM,
                  WN = Cfg::WN, PLANE = Cfg::PLANE, NWP = Cfg::NWP, NWPASS = Cfg::NWPASS;
    extern __shared__ __attribute__((aligned(16))) char smem_x3s[];
    char* const Pb = smem_x3s;

    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int rr = id >> 3;
    const int ct = rr % a.nct;
    // every XCD walks its own contiguous, row-major range of pixel tiles (conv_x3h.hip: neighbours share halo lines in the XCD's L2)
    const int per_xcd = (a.npt + 7) >> 3;
    const int pt = xcd * per_xcd + rr / a.nct;
    if (pt >= a.npt) return;
    const int tiles_per_img = a.tiles_h * a.tiles_w;
    const int n = pt / tiles_per_img;
    const int trem = pt - n * tiles_per_img;
    const int h0 = (trem / a.tiles_w) * TH;
    const int w0 = (trem % a.tiles_w) * TW;
    const int co0 = ct * MT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchunk = (a.Cin + 7) >> 3;
    const unsigned lds0 = (unsigned)(size_t)smem_x3s;

    // ---- this thread's column pairs of the halo tile: byte offset of the pair's even column in a channel plane (2^31: padding) ----
    const unsigned xsH4 = (unsigned)a.src[0].sH * 4u;
    int xvo[NPASS];
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        const int s = p * 256 + tid;
        const int r = s / RUN, u = s - r * RUN;
        const int hi = 2 * h0 - 1 + r, wi = 2 * w0 - 2 + 2 * u;             // (Win is even: column wi + 1 is inside whenever wi is)
        const bool ok = s < NSLOT && hi >= 0 && hi < a.Hin && wi >= 0 && wi < a.Win;
        xvo[p] = ok ? (int)((unsigned)hi * xsH4 + (unsigned)(wi * 4)) : (int)0x80000000u;
    }
    // ---- weight operands: LDS order [tap][plane][m], source x3w[chunk][(tap * 2 + plane) * CoutPad + co0 + m] (conv_x3h.hip) ----
    unsigned woff0;
    {
        const int q = wave * 64 + lane;
        const int m = q % MT, tp = q / MT;
        woff0 = (unsigned)((tp * a.CoutPad + m) * 16);
    }
    const unsigned wstep = (unsigned)((256 / MT) * a.CoutPad * 16);   // four waves further on
    const long long wchunk_bytes = (long long)KK * 2 * a.CoutPad * 16;
    auto issue_w = [&](int k) {                                    // the weight DMA of chunk k: NWPASS wave-instructions
        const char* wb = static_cast<const char*>(a.x3w) + k * wchunk_bytes + (long long)co0 * 16;
        const i32x4 wr = make_rsrc(reinterpret_cast<const float*>(wb), (unsigned)(wchunk_bytes - (long long)co0 * 16));
        const unsigned ws_b = lds0 + (unsigned)(Cfg::P_BYTES + (k & 1) * Cfg::W_BYTES);
#pragma unroll
        for (int i = 0; i < NWPASS; ++i) {
            const int pp = wave + 4 * i;
            if ((pp + 1) * 64 <= NWP) dma16s(ws_b + pp * 1024, woff0, wr, (unsigned)i * wstep);
            else if (pp * 64 + lane < NWP) dma16s(ws_b + pp * 1024, woff0, wr, (unsigned)i * wstep);
        }
    };
    // Pixel registers of two chunks: the loads of chunk k+2 are issued during the multiply phase of chunk k and consumed at the end of
    // the multiply phase of chunk k+1.  Every chunk issues the SAME number of loads (channels beyond Cin read through an empty
    // descriptor), so the hand-placed s_waitcnt counts are compile-time constants.
    const float* xp = a.src[0].p + (long long)n * a.src[0].sN;
    const long long xsC = a.src[0].sC;
    vr_f32x2s xr[2][NPASS][8];                                     // (.x: the even column -> O run, .y: the odd column -> E run)
    auto load_channel = [&](int k, int cl, auto par) {
        constexpr int PAR = decltype(par)::value;
        const int ci = k * 8 + cl;                                // wave-uniform
        const bool live = ci < a.Cin;
        const i32x4 xs = make_rsrc(xp, live ? 0x7FFFFFF0u : 0u);
#pragma unroll
        for (int p = 0; p < NPASS; ++p) xr[PAR][p][cl] = x3s_load2(xs, xvo[p]);
        if (live) xp += xsC;
    };
    // the pixel registers of set PAR have landed when at most NEWER younger vector-memory operations are outstanding
    auto wait_pixels = [&](auto par, auto newer) {
        constexpr int PAR = decltype(par)::value, NEWER = decltype(newer)::value;
#pragma unroll
        for (int p = 0; p < NPASS; ++p) x3s_wait8<NEWER>(xr[PAR][p]);
    };
    // ---- the running power-of-two shift of the pixels (conv_x3h.hip): x' = x * 2^sh ----
    int sh = 0, shlo = 0;                                          // (shlo: the shift the largest chunk so far asked for)
    float psc = 1.f;                                               // 2^sh
    // max |x| over this thread's pixel registers of set PAR -> wave maximum -> LDS (read back behind the next barrier)
    auto post_max = [&](auto par) {
        constexpr int PAR = decltype(par)::value;
        float m = 0.f;
#pragma unroll
        for (int p = 0; p < NPASS; ++p)
#pragma unroll
            for (int cl = 0; cl < 8; ++cl)         // (inline asm: hipcc canonicalises fabsf() with a v_max of its own per value)
                asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(xr[PAR][p][cl].x), "v"(xr[PAR][p][cl].y));
        int b = __float_as_int(m);                                 // non-negative floats order like their bit patterns
        b = max(b, __builtin_amdgcn_update_dpp(0, b, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
        b = max(b, __builtin_amdgcn_update_dpp(0, b, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
        b = max(b, __builtin_amdgcn_update_dpp(0, b, 0x141, 0xF, 0xF, true));   // row_half_mirror
        b = max(b, __builtin_amdgcn_update_dpp(0, b, 0x140, 0xF, 0xF, true));   // row_mirror: every lane of a row of 16 holds the row's maximum
        const int w = max(max(__builtin_amdgcn_readlane(b, 0), __builtin_amdgcn_readlane(b, 16)),
                          max(__builtin_amdgcn_readlane(b, 32), __builtin_amdgcn_readlane(b, 48)));
        if (lane == 0) reinterpret_cast<int*>(smem_x3s + Cfg::M_OFF)[wave] = w;
    };
    auto read_max_exp = [&]() -> int {
        const vr_i32x4 mm = *reinterpret_cast<const vr_i32x4*>(smem_x3s + Cfg::M_OFF);
        const int w = max(max(mm[0], mm[1]), max(mm[2], mm[3]));
        return __builtin_amdgcn_readfirstlane(w) >> 23;            // biased exponent of the largest |x| (255: inf / nan)
    };
    // split the chunk's pixels into the two fp16 planes, parity runs apart
    auto convert = [&](auto par) {
        constexpr int PAR = decltype(par)::value;
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int s = p * 256 + tid;
            if ((p + 1) * 256 <= NSLOT || s < NSLOT) {
                const int r = s / RUN, u = s - r * RUN;
                vr_i32x4 eh, el, oh, ol;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int h, l;
                    split2h_pair(xr[PAR][p][2 * j].y, xr[PAR][p][2 * j + 1].y, psc, h, l);
                    eh[j] = h; el[j] = l;
                    split2h_pair(xr[PAR][p][2 * j].x, xr[PAR][p][2 * j + 1].x, psc, h, l);
                    oh[j] = h; ol[j] = l;
                }
                char* q = Pb + (r * RP + u) * 16;
                *reinterpret_cast<vr_i32x4*>(q) = eh;
                *reinterpret_cast<vr_i32x4*>(q + PLANE) = el;
                *reinterpret_cast<vr_i32x4*>(q + RUN * 16) = oh;
                *reinterpret_cast<vr_i32x4*>(q + RUN * 16 + PLANE) = ol;
            }
        }
    };

    const int khalf = lane >> 5, l31 = lane & 31;
    // B operands: output pixel (row wave*WN + ni, column l31), tap (ty, tx), plane 0: bq + ((2 ni + ty) * RP + ex(tx)) * 16.
    //   X(t): lanes 0-31 plane 0 (b1), lanes 32-63 plane 1 (b2) of tap t's pixel;   Y(t,t+1): plane 0, lanes 32-63 at tap t+1's pixel:
    //   a constant entry distance per pair -- (0,1) and (6,7): O[j+1] - E[j];  (2,3): next row's E[j] - E[j+1];  (4,5): E[j+1] - O[j+1]
    const int bq = (2 * wave * WN * RP + l31) * 16;
    const int bX = bq + khalf * PLANE;
    const int bYa = bq + khalf * (Cfg::ex(1) - Cfg::ex(0)) * 16, bYb = bq + khalf * (RP + Cfg::ex(0) - Cfg::ex(2)) * 16,
              bYc = bq - khalf * (Cfg::ex(1) - Cfg::ex(2)) * 16;
    // A operands, LDS order [tap][plane][m]:  X(t): a1(t) in both halves;  Y(t,t+1): a2(t) | a2(t+1);  Y(8): a2(8) | 0
    const int aX = l31 * 16, aY = (MT + l31 + khalf * 2 * MT) * 16;

    f32x16 acc[WM][WN];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    // epilogue constants of this cout tile (bias; folded BatchNorm scale / shift; 1 / weight scale): loaded FIRST, parked in LDS
    // behind the first pixel wait
    float ecv[4];
    {
        const int ec = co0 + (tid & (MT - 1));
        const int ecc = ec < a.Cout ? ec : a.Cout - 1;
        const i32x4 rb = make_rsrc(a.bias, a.bias ? 0x7FFFFFF0u : 0u);
        const i32x4 re = make_rsrc(a.epi, a.epi ? 0x7FFFFFF0u : 0u);
        const i32x4 rw = make_rsrc(reinterpret_cast<const float*>(static_cast<const char*>(a.x3w) + nchunk * wchunk_bytes), 0x7FFFFFF0u);
        ecv[0] = x3h_load(rb, ecc * 4);
        ecv[1] = x3h_load(re, ecc * 8);
        ecv[2] = x3h_load(re, ecc * 8 + 4);
        ecv[3] = x3h_load(rw, ec * 4);                                             // (padded couts included: [CoutPad])
    }
    // the shift follows the chunk maxima, unchanged from conv_x3h.hip: `e` = biased exponent of the largest |x| of the chunk about to be split
    auto follow = [&](int e, bool first) {
        const int need = 140 - (e < 14 ? 14 : e);                                  // chunk maximum -> [2^13, 2^14)
        shlo = (first || need < shlo) ? need : shlo;
        int nsh = sh;
        if (first || need < sh - 1) nsh = need;                                    // (larger than 2^15 after scaling: must move)
        else if (need > sh + 12) {                                                 // (maximum below 2: the second plane starts losing bits)
            nsh = need < sh + 64 ? need : sh + 64;
            nsh = nsh < shlo + 64 ? nsh : shlo + 64;
            nsh = nsh > sh ? nsh : sh;
        }
        if (nsh != sh) {
            if (!first) {
                const int d = nsh - sh;                                            // <= 64; a large negative d flushes the old sums
                const float f = d < -126 ? 0.f : x3h_pow2(d);
#pragma unroll
                for (int mi = 0; mi < WM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[mi][ni][r] *= f;
            }
            sh = nsh;
            psc = x3h_pow2(sh);                                                    // sh in [-115, 126]
        }
    };
    // prologue: pixels of chunk 0 -> P, weights of chunk 0 and pixels of chunk 1 in flight
#pragma unroll
    for (int cl = 0; cl < 8; ++cl) load_channel(0, cl, P0{});
    issue_w(0);
#pragma unroll
    for (int cl = 0; cl < 8; ++cl) load_channel(1, cl, P1{});
    wait_pixels(P0{}, std::integral_constant<int, Cfg::NXL + Cfg::NWMIN>{});      // chunk 0's pixels (weights and chunk 1 stay in flight)
    asm volatile("; landed %0 %1 %2 %3" : "+v"(ecv[0]), "+v"(ecv[1]), "+v"(ecv[2]), "+v"(ecv[3]));      // (older loads: landed with them; the comment is for tools/asm_inflight_audit2.py)
    if (tid < MT) {
        float* E = reinterpret_cast<float*>(smem_x3s + Cfg::E_OFF);
        E[tid] = ecv[0];
        E[MT + tid] = a.epi ? ecv[1] : 1.f;
        E[2 * MT + tid] = a.epi ? ecv[2] : 0.f;
        E[3 * MT + tid] = ecv[3];
    }
    post_max(P0{});
    lds_barrier();
    follow(read_max_exp(), true);
    convert(P0{});
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(Cfg::NXL) : "memory");   // weights of chunk 0 landed; chunk 1's pixels stay in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // one chunk: multiply P(k) x W(k) while the weights of chunk k+1 and the pixels of chunk k+2 arrive; then split chunk k+1 into P
    auto chunk = [&](int k, auto par) {
        constexpr int PAR = decltype(par)::value;                 // k & 1: the pixel registers chunk k came from (free again)
        const bool more = k + 1 < nchunk;
        {
            const char* Wb = smem_x3s + Cfg::P_BYTES + PAR * Cfg::W_BYTES;
            vr_f16x8 A[2][WM], B[2][WN];
            // group g of the 14: g = 3q + {0, 1} -> X(2q), X(2q + 1); g = 3q + 2 -> Y(2q, 2q + 1); g = 12 -> X(8); g = 13 -> Y(8)
            auto read_group = [&](int g, int buf) {
                const bool isY = g == 13 || (g < 12 && g % 3 == 2);
                const int t = g >= 12 ? 8 : 2 * (g / 3) + (g % 3 == 1 ? 1 : 0);
                const int ty = t / 3, tx = t % 3;
#pragma unroll
                for (int mi = 0; mi < WM; ++mi) {
                    const char* q = Wb + (t * 2 * MT + mi * 32) * 16;
                    if (!isY) A[buf][mi] = *reinterpret_cast<const vr_f16x8*>(q + aX);
                    else if (t < 8) A[buf][mi] = *reinterpret_cast<const vr_f16x8*>(q + aY);
                    else {
                        const vr_i32x4 v = *reinterpret_cast<const vr_i32x4*>(q + aX + MT * 16);
                        vr_i32x4 z;
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j] = khalf ? 0 : v[j];
                        A[buf][mi] = __builtin_bit_cast(vr_f16x8, z);
                    }
                }
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    const int o = ((2 * ni + ty) * RP + Cfg::ex(tx)) * 16;
                    if (!isY) B[buf][ni] = *reinterpret_cast<const vr_f16x8*>(Pb + bX + o);
                    else if (t == 8) B[buf][ni] = *reinterpret_cast<const vr_f16x8*>(Pb + bq + o);     // (upper half meets zeros)
                    else if (t == 2) B[buf][ni] = *reinterpret_cast<const vr_f16x8*>(Pb + bYb + o);
                    else if (t == 4) B[buf][ni] = *reinterpret_cast<const vr_f16x8*>(Pb + bYc + o);
                    else B[buf][ni] = *reinterpret_cast<const vr_f16x8*>(Pb + bYa + o);
                }
            };
            auto mfma_group = [&](int buf) {
#pragma unroll
                for (int mi = 0; mi < WM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni) acc[mi][ni] = mfma_f16x16(A[buf][mi], B[buf][ni], acc[mi][ni]);
            };
            read_group(0, 0);
#pragma unroll
            for (int g = 0; g < Cfg::NG; ++g) {
                const int cur = g & 1;
                // the operand reads of group g+1 go out in front of the matrix instructions of group g; the vector-memory work for the
                // coming chunks rides behind the first groups (weights first: they are needed one chunk earlier)
                if (g + 1 < Cfg::NG) read_group(g + 1, cur ^ 1);
                if (more) {
                    if (g == 0) issue_w(k + 1);
                    if (g >= 1 && g <= 4) { load_channel(k + 2, 2 * g - 2, par); load_channel(k + 2, 2 * g - 1, par); }
                }
                __builtin_amdgcn_sched_barrier(0);
                mfma_group(cur);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (more) {
            using Q = std::integral_constant<int, PAR ^ 1>;
            // outstanding, oldest first: chunk k+1's pixels | weights of chunk k+1 | chunk k+2's pixels
            wait_pixels(Q{}, std::integral_constant<int, Cfg::NXL + Cfg::NWMIN>{});
            post_max(Q{});
            lds_barrier();                                       // every wave has read P(k); the maxima of chunk k+1 are in LDS
            follow(read_max_exp(), false);
            convert(Q{});
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(Cfg::NXL) : "memory");   // weights of chunk k+1 landed
            __builtin_amdgcn_s_barrier();                        // P(k+1) complete
            asm volatile("" ::: "memory");
        }
    };
    for (int k = 0; k < nchunk; k += 2) {
        chunk(k, P0{});
        if (k + 1 < nchunk) chunk(k + 1, P1{});
    }
    // The last prefetch targets channels beyond Cin through an empty descriptor: nothing waits for those zero-returning loads inside
    // the loop, and hipcc does not track inline-asm loads -- drain them before the epilogue may reuse the xr[] registers.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---------------- epilogue (conv_epilogue.h): bias, BatchNorm + activation, up to three destination segments ---------
    {
        // undo the two scalings: 2^-sh (pixels, this workgroup) and 1 / weight scale (per cout: E[3][m], row m = mi*32 + (r&3) + 8*(r>>2) + 4*khalf)
        const float fo = x3h_pow2(-sh);                           // sh in [-115, 126]
        const float* Wi = reinterpret_cast<const float*>(smem_x3s + Cfg::E_OFF) + 3 * MT;
#pragma unroll
        for (int mi = 0; mi < WM; ++mi)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const vr_f32x4h wi = *reinterpret_cast<const vr_f32x4h*>(Wi + mi * 32 + 8 * rq + 4 * khalf);
#pragma unroll
                for (int ni = 0; ni < WN; ++ni)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][ni][rq * 4 + j] = (acc[mi][ni][rq * 4 + j] * fo) * wi[j];
            }
    }
    {
        int hon[WN], won[WN];
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) { hon[ni] = h0 + wave * WN + ni; won[ni] = w0 + l31; }
        epi_store<MT, WM, WN>(VR_EPI_ARGS(a), acc, reinterpret_cast<const float*>(smem_x3s + Cfg::E_OFF), n, co0, khalf,
                              h0 + TH <= a.Hout && w0 + TW <= a.Wout, hon, won);
    }
}

template <int MT, int TH>
static void x3s_launch(const ConvArgs& a, hipStream_t st) {
    using Cfg = X3sCfg<MT, TH>;
    auto kern = conv_x3h_kernel_s2<MT, TH>;
    static std::atomic<unsigned long long> attr_done{0};
    ensure_lds_attr(attr_done, reinterpret_cast<const void*>(kern), Cfg::LDS_BYTES);
    const int groups = (a.npt + 7) / 8;
    VR_LAUNCH(kern, dim3(groups * 8 * a.nct), dim3(256), Cfg::LDS_BYTES, st, a);
    VR_HIP(hipGetLastError());
}

// True when the launch can take this kernel: mfma_mode 3, eval, 3x3 stride 2 pad 1, one plain source whose column pairs are whole
// and 8-byte aligned, at least 32 output columns.  The tile choice depends on the launch's shape alone.
bool x3s_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p) {
    if (a.bf16 != 3 || !a.x3w || a.tapmask || a.part || a.w_hi != 0 || a.nsrc != 1) return false;
    if (!(s.KS == 3 && s.stride == 2 && s.dil_h == 1 && s.dil_w == 1) || a.pad_h != 1 || a.pad_w != 1) return false;
    if (a.Hin < 1 || a.Hout != (a.Hin - 1) / 2 + 1 || a.Wout != (a.Win - 1) / 2 + 1 || a.Wout < 32) return false;
    const ConvSrc& c = a.src[0];
    if (!conv_src_plain(c) || c.up || c.W != a.Win || c.H != a.Hin) return false;
    // dwordx2 loads of (even, odd) column pairs: no pair may straddle the right edge, every pair 8-byte aligned
    if ((a.Win & 1) || (c.sH & 1) || (c.sC & 1) || (c.sN & 1) || (reinterpret_cast<unsigned long long>(c.p) & 7)) return false;
    if ((long long)c.H * (c.sH > 0 ? c.sH : 1) * 4 >= 0x7FFFFFF0LL) return false;
    // One or two chunks never fill the two-chunks-ahead pipeline: the launch is its prologue, and conv_dma.hip (more workgroups per CU) is
    // as fast or faster at the 6 + 5 crop grids the executor lanes launch.  Measured per launch, conv_dma -> this kernel, 6 / 5 crops
    // (profiles/x3s_infer_ab.md): ci8 co16 256x128 17.8 -> 21.5 / 17.5 -> 20.8 us; ci16 co32 256x128 25.8 -> 28.6 / 25.8 -> 24.8 and
    // 25.6 -> 28.4 / 25.1 -> 24.6; ci16 co32 128x64 13.8 -> 13.0 / 13.5 -> 13.0.  The network's next layers (ci32: four chunks) gain 14 % or more.
    if (a.Cin <= 16) return false;
    int MT = (a.CoutPad % 64 == 0) ? 64 : 32;
    const long long tiles8 = (long long)a.N * ((a.Hout + 7) / 8) * ((a.Wout + 31) / 32);
    if (MT == 64 && tiles8 * (a.CoutPad / 64) < 512) MT = 32;            // fewer than two workgroups per CU: halve the cout tile
    *p = ConvPlan{CK_X3S, MT, 8, 32, nullptr};
    return true;
}

void x3s_launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    if (p.MT == 64) x3s_launch<64, 8>(a, st);
    else x3s_launch<32, 8>(a, st);
}

}  // namespace vr
