// The second, 1x1 stage conv_x3h.hip can run on its accumulators (ConvArgs::tail): the stage tails of the low-band nets and the LSTM
// squeeze.  Included by conv_x3h.hip alone.
#pragma once
#include "conv_epilogue.h"
#include "x3h_common.h"

namespace vr {

// ---- a second 1x1 stage on the accumulators (ConvArgs::tail; conv_x3h.hip, one cout tile per workgroup, eval) --------------------
// A lane holds, for ITS pixel column, the couts mi*32 + (r&3) + 8*(r>>2) + 4*khalf; lane ^ 32 holds the other half of the channels of
// the same pixel: channels 4s .. 4s+3 (segment s) live in half s & 1.  Both forms sum over the channels IN ORDER, c = 0, 1, 2, ..., one
// fp32 fma each from 0 -- the order of the kernels that run the stage as a launch of its own (thin_conv_kernel's loop, the k chain of
// conv_dma's fp32 matrix instructions), so fusing the stage does not reassociate its sum.
// Every LDS return (constants, ds_bpermute) is waited for in full before its first consumer (hardware fact 5).
typedef float vr_epi_f4 __attribute__((ext_vector_type(4)));

// lane ^ 32's values of v[0..K-1]
template <int K>
__device__ __forceinline__ void x3h_other_half(const float (&v)[K], float (&o)[K], int lane) {
    const int addr = (lane ^ 32) * 4;
#pragma unroll
    for (int i = 0; i < K; ++i)                                // (asm: stays in program order with the waits and the pinned sums around it)
        asm volatile("ds_bpermute_b32 %0, %1, %2" : "=v"(o[i]) : "v"(addr), "v"(v[i]));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < K; ++i) asm volatile("" : "+v"(o[i]));
}

// TAIL 1, J = 8 or 16 output channels: the halves swap their ACTIVATIONS once (16 x WN values), then the lower half-wave computes outputs
// 0 .. J/2-1 and the upper J/2 .. J-1 of its pixels, each over all 32 channels.  T = w2 [32][16] | affine [16][2]
template <int WN, int J>
__device__ __forceinline__ void x3h_tail_mix(f32x16 (&acc)[1][WN], const float* T, float tslope, int tCout, float* tp, long long tsN,
                                             long long tsC, long long tsH, int n, int hrow0, int wcol, int Hout, int Wout, int khalf, int lane) {
    constexpr int H = J / 2, CB = 32 / H;                       // outputs per lane; channels per batch of weight reads (32 registers)
    constexpr int NP = 2;                                      // pixel groups per pass (register budget: 16 NP received values + H NP sums)
    static_assert(WN % NP == 0, "pixel groups");
    float s2[H], b2[H];
#pragma unroll
    for (int jj = 0; jj < H; ++jj) {
        s2[jj] = T[512 + 2 * (khalf * H + jj)];
        b2[jj] = T[512 + 2 * (khalf * H + jj) + 1];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int jj = 0; jj < H; ++jj) asm volatile("" : "+v"(s2[jj]), "+v"(b2[jj]));
    float* const q0 = tp + (long long)n * tsN + (long long)(khalf * H) * tsC + wcol;
    const unsigned wl = (unsigned)(size_t)T + (unsigned)(khalf * H * 4);      // LDS byte address of this half's outputs in row 0 of w2
    // (static_for: a loop `#pragma unroll` leaves rolled would index the register arrays at run time, i.e. keep them in scratch)
    static_for<WN / NP>([&](auto pass) {
        constexpr int n0 = decltype(pass)::value * NP;
        float mine[16 * NP], oth[16 * NP];
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int ni = 0; ni < NP; ++ni) mine[r * NP + ni] = acc[0][n0 + ni][r];
        x3h_other_half<16 * NP>(mine, oth, lane);
        // segment 2 rq (channels 8 rq + j) is the lower half's, 2 rq + 1 (8 rq + 4 + j) the upper's: register rq * 4 + j of the owner
        float y[H][NP];
#pragma unroll
        for (int jj = 0; jj < H; ++jj)
#pragma unroll
            for (int ni = 0; ni < NP; ++ni) y[jj][ni] = 0.f;
        static_for<32 / CB>([&](auto batch) {
            constexpr int cb = decltype(batch)::value;
            // (inline asm: as plain loads hipcc hoists the weight reads of ALL batches in front of the first fma -- 256 registers.  The
            // vectors are released behind the wait, before anything takes them apart.)
            vr_epi_f4 q[CB][H / 4];
#pragma unroll
            for (int i = 0; i < CB; ++i)
#pragma unroll
                for (int j4 = 0; j4 < H / 4; ++j4)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(q[i][j4]) : "v"(wl), "n"(((cb * CB + i) * 16 + 4 * j4) * 4));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            float w[CB][H];
#pragma unroll
            for (int i = 0; i < CB; ++i)
#pragma unroll
                for (int j4 = 0; j4 < H / 4; ++j4) {
                    asm volatile("" : "+v"(q[i][j4]));
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[i][4 * j4 + e] = q[i][j4][e];
                }
            static_for<CB>([&](auto ch) {
                constexpr int i = decltype(ch)::value, c = cb * CB + i;
                constexpr int r = (c >> 3) * 4 + (c & 3);
                constexpr bool upper = ((c >> 2) & 1) != 0;     // the segment's owner
#pragma unroll
                for (int ni = 0; ni < NP; ++ni) {
                    float av = (upper == (khalf != 0)) ? mine[r * NP + ni] : oth[r * NP + ni];
                    asm volatile("" : "+v"(av));                // (keeps the select behind its batch's wait)
#pragma unroll
                    for (int jj = 0; jj < H; ++jj) y[jj][ni] = fmaf(w[i][jj], av, y[jj][ni]);
                }
            });
            // (the sums are pinned behind their batch: left free, hipcc sinks every fma below the LAST batch's reads and spills the weights)
#pragma unroll
            for (int jj = 0; jj < H; ++jj)
#pragma unroll
                for (int ni = 0; ni < NP; ++ni) asm volatile("" : "+v"(y[jj][ni]));
        });
#pragma unroll
        for (int jj = 0; jj < H; ++jj)
#pragma unroll
            for (int ni = 0; ni < NP; ++ni) {
                const float v = act_apply(fmaf(y[jj][ni], s2[jj], b2[jj]), tslope);
                const int ho = hrow0 + n0 + ni;
                if (khalf * H + jj < tCout && ho < Hout && wcol < Wout) q0[(long long)jj * tsC + (long long)ho * tsH] = v;
            }
    });
}

// acc: conv sums, un-scaled (TAIL 2: epi_store has run, so the bias is already in).  E: the first stage's constants [4][MT];
// T: the second stage's (X3hCfg::T_OFF).  hrow0 / wcol: output row of pixel group 0 / output column of this lane.
template <int MT, int WM, int WN, int TAIL>
__device__ __forceinline__ void x3h_second_stage(f32x16 (&acc)[WM][WN], const float* E, const float* T, float eslope, float tslope, int tCout, float* tp,
                                         long long tsN, long long tsC, long long tsH, int n, int hrow0, int wcol, int Hout, int Wout, int khalf,
                                         int lane) {
    static_assert(TAIL == 2 || (MT == 32 && WM == 1), "the stage tail takes one 32-cout block");
    // the first stage's own bias, folded BatchNorm and activation, in place: what epi_store computes on the way out, to the bit
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const int cb = mi * 32 + 8 * rq + 4 * khalf;
            const vr_epi_f4 b4 = *reinterpret_cast<const vr_epi_f4*>(E + cb), s4 = *reinterpret_cast<const vr_epi_f4*>(E + MT + cb),
                            h4 = *reinterpret_cast<const vr_epi_f4*>(E + 2 * MT + cb);
            float eb[4], esc[4], esh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { eb[j] = b4[j]; esc[j] = s4[j]; esh[j] = h4[j]; }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(eb[j]), "+v"(esc[j]), "+v"(esh[j]));
#pragma unroll
            for (int ni = 0; ni < WN; ++ni)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = acc[mi][ni][rq * 4 + j];
                    if constexpr (TAIL == 1) v += eb[j];
                    acc[mi][ni][rq * 4 + j] = act_apply(fmaf(v, esc[j], esh[j]), eslope);
                }
        }
    if constexpr (TAIL == 1) {
        if (tCout <= 8) x3h_tail_mix<WN, 8>(acc, T, tslope, tCout, tp, tsN, tsC, tsH, n, hrow0, wcol, Hout, Wout, khalf, lane);
        else x3h_tail_mix<WN, 16>(acc, T, tslope, tCout, tp, tsN, tsC, tsH, n, hrow0, wcol, Hout, Wout, khalf, lane);
    } else {
        // the LSTM squeeze: one channel, BatchNorm + ReLU, 32 consecutive floats per row.  T = w2 [MT] | (scale, shift)
        float wv[WM * 16];
#pragma unroll
        for (int mi = 0; mi < WM; ++mi)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const vr_epi_f4 q = *reinterpret_cast<const vr_epi_f4*>(T + mi * 32 + 8 * rq + 4 * khalf);
#pragma unroll
                for (int j = 0; j < 4; ++j) wv[mi * 16 + rq * 4 + j] = q[j];
            }
        float s2 = T[MT], b2 = T[MT + 1];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < WM * 16; ++i) asm volatile("" : "+v"(wv[i]));
        asm volatile("" : "+v"(s2), "+v"(b2));
        // the sum walks the channels in order, so it changes sides after every segment of four: 8 WM - 1 hand-overs of WN values
        float z[WN];
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) z[ni] = 0.f;
#pragma unroll
        for (int sg = 0; sg < 8 * WM; ++sg) {
            const int mi = sg >> 3, rq = (sg & 7) >> 1;
            const bool owner = (khalf != 0) == ((sg & 1) != 0);
            if (sg > 0) {                                       // the running sum arrives from the previous segment's owner
                float zo[WN];
                x3h_other_half<WN>(z, zo, lane);
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) z[ni] = owner ? zo[ni] : z[ni];
            }
#pragma unroll
            for (int ni = 0; ni < WN; ++ni) {
                float t = z[ni];
#pragma unroll
                for (int j = 0; j < 4; ++j) t = fmaf(wv[mi * 16 + rq * 4 + j], acc[mi][ni][rq * 4 + j], t);
                z[ni] = owner ? t : z[ni];
            }
        }
        float* const q0 = tp + (long long)n * tsN + wcol;       // (the last segment is the upper half's)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) {
            const float v = fmaxf(fmaf(z[ni], s2, b2), 0.f);
            if (khalf && hrow0 + ni < Hout && wcol < Wout) q0[(long long)(hrow0 + ni) * tsH] = v;
        }
    }
}

}  // namespace vr
