// The two matrix products of layers.LSTMModule in eval (lib/layers.py:117-133): the LSTM input projection and the Linear behind the LSTM,
//   out[n][co][t] = act((sum_k W[k][co] x[n][k][t] + b[co]) * scale[co] + shift[co]),      x [N][K][T], W [K][CoutPad], out [N][Cout][T].
// As 1x1 convs on a one-row image they took conv_dma.hip's 8-row x 32-column x 32-cout tile: 64 - 128 workgroups on 256 CUs, each walking
// K in 16-channel chunks, one memory round trip per chunk (25.8 us for 0.18 GFLOP, profiles/fused_tail_infer_per_launch.txt).
//
// Here the output is cut into tiles of (16 MC) couts x (16 NP) positions, positions counted over (n, t) flattened; the host takes the
// largest of 32 x 32, 32 x 16 and 16 x 16 that still makes two workgroups per CU (5 crops of 128 frames and 256 couts: 640 tiles of
// 16 x 16).  A workgroup is four waves; wave w owns the w-th quarter of K and walks it in ascending k with v_mfma_f32_16x16x4_f32 (fp32
// operands, fp32 accumulate), its operands loaded straight into the instruction's layout -- lane = (cout or position) + 16 * (k % 4):
// 64-byte runs of W's rows and of x's rows -- in batches of 16 steps, every load of a batch issued before its first product.  K = 256 is
// ONE batch per wave, K = 512 two.  The four partial tiles meet in LDS and are added in wave order; bias, folded BatchNorm and activation
// as conv_epilogue.h applies them.  No atomics, and a value depends on neither its tile nor the tiling: the same inputs give the same bits.
// Out-of-range lanes (k >= K, co >= Cout, position >= N T) load a clamped, valid address and are zeroed in registers: the padded
// weight columns are never read.
#include "conv_stage.h"
#include "kernels.h"

namespace vr {

typedef float rg_f32x4 __attribute__((ext_vector_type(4)));

// v where keep, else +0: a bit mask, not a select -- behind a select hipcc loads under the condition and waits for every load on its own
__device__ __forceinline__ float rg_keep(float v, bool keep) { return __uint_as_float(__float_as_uint(v) & (keep ? 0xFFFFFFFFu : 0u)); }

template <int MC, int NP>
__global__ __launch_bounds__(256) void rows_gemm_kernel(const RowsGemmArgs a) {
    constexpr int NB = 16;                                        // steps of 4 k per batch
    constexpr int NS = MC * NP;                                   // 16 x 16 sub-tiles, j = mc * NP + np
    __shared__ float red[4][NS][4][64];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    const int P = a.N * a.T;
    const int co0 = blockIdx.y * (16 * MC), p0 = blockIdx.x * (16 * NP);
    const float* wb[MC];
    bool cok[MC];
#pragma unroll
    for (int mc = 0; mc < MC; ++mc) {
        const int co = co0 + 16 * mc + l16;
        cok[mc] = co < a.Cout;
        wb[mc] = a.w + (cok[mc] ? co : a.Cout - 1);
    }
    const float* xb[NP];
    bool pok[NP];
    long long ob[NP];                                             // out offset of (n, cout 0, t)
#pragma unroll
    for (int np = 0; np < NP; ++np) {
        const int p = p0 + 16 * np + l16;
        pok[np] = p < P;
        const int pc = pok[np] ? p : P - 1;
        const int n = pc / a.T, t = pc - n * a.T;
        xb[np] = a.x + (long long)n * a.xN + t;
        ob[np] = (long long)n * a.Cout * a.T + t;
    }

    const int nsteps = (a.K + 3) >> 2;
    const int per = (nsteps + 3) >> 2;
    const int sbeg = wave * per;
    const int send = min(sbeg + per, nsteps);

    rg_f32x4 acc[MC][NP];
#pragma unroll
    for (int mc = 0; mc < MC; ++mc)
#pragma unroll
        for (int np = 0; np < NP; ++np) acc[mc][np] = rg_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = sbeg; s0 < send; s0 += NB) {
        float av[MC][NB], bv[NP][NB];
        // every load of the batch first, from clamped addresses ...
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = (s0 + i) * 4 + kq;
            const int kc = s0 + i < send && k < a.K ? k : a.K - 1;
#pragma unroll
            for (int mc = 0; mc < MC; ++mc) av[mc][i] = wb[mc][(long long)kc * a.CoutPad];
#pragma unroll
            for (int np = 0; np < NP; ++np) bv[np][i] = xb[np][(long long)kc * a.T];
        }
        __builtin_amdgcn_sched_barrier(0);                        // (left alone, hipcc weaves the products between the loads and waits for each)
        // ... then the products, the out-of-range operands zeroed as they are used
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const bool kok = s0 + i < send && (s0 + i) * 4 + kq < a.K;
            float am[MC], bm[NP];
#pragma unroll
            for (int mc = 0; mc < MC; ++mc) am[mc] = rg_keep(av[mc][i], kok && cok[mc]);
#pragma unroll
            for (int np = 0; np < NP; ++np) bm[np] = rg_keep(bv[np][i], kok && pok[np]);
#pragma unroll
            for (int mc = 0; mc < MC; ++mc)
#pragma unroll
                for (int np = 0; np < NP; ++np) acc[mc][np] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[mc], bm[np], acc[mc][np], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mc = 0; mc < MC; ++mc)
#pragma unroll
        for (int np = 0; np < NP; ++np)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][mc * NP + np][r][lane] = acc[mc][np][r];
    __syncthreads();
    // sub-tile j is finished by wave j % 4: the four partial sums in wave order; accumulator row r of lane (l16, kq) is cout 4 kq + r of
    // the sub-tile, column l16 its position
#pragma unroll
    for (int mc = 0; mc < MC; ++mc)
#pragma unroll
        for (int np = 0; np < NP; ++np) {
            const int j = mc * NP + np;
            if ((j & 3) != wave) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = co0 + 16 * mc + 4 * kq + r;
                float v = ((red[0][j][r][lane] + red[1][j][r][lane]) + red[2][j][r][lane]) + red[3][j][r][lane];
                if (c < a.Cout && pok[np]) {
                    if (a.bias) v += a.bias[c];
                    if (a.epi) v = act_apply(fmaf(v, a.epi[2 * c], a.epi[2 * c + 1]), a.slope);
                    a.out[ob[np] + (long long)c * a.T] = v;
                }
            }
        }
}

bool rows_gemm_ok(const RowsGemmArgs& a) {
    if (!a.x || !a.w || !a.out) return false;
    if (a.N < 1 || a.T < 1 || a.K < 1 || a.Cout < 1 || a.CoutPad < a.Cout) return false;
    if ((long long)a.N * a.T > 0x7FFFFFF0LL / 16 || a.xN < (long long)a.K * a.T) return false;
    return (a.Cout + 15) / 16 <= 65535;                           // blockIdx.y
}

// the largest tile that still gives two workgroups per CU, else the smallest
int rows_gemm_tile(const RowsGemmArgs& a) {
    const long long P = (long long)a.N * a.T;
    auto groups = [&](int mc, int np) { return ((P + 16 * np - 1) / (16 * np)) * ((a.Cout + 16 * mc - 1) / (16 * mc)); };
    if (groups(2, 2) >= 512) return 22;
    if (groups(2, 1) >= 512) return 21;
    return 11;
}

template <int MC, int NP>
static void rows_gemm_launch(const RowsGemmArgs& a, hipStream_t st) {
    const int P = a.N * a.T;
    VR_LAUNCH((rows_gemm_kernel<MC, NP>), dim3((unsigned)((P + 16 * NP - 1) / (16 * NP)), (unsigned)((a.Cout + 16 * MC - 1) / (16 * MC))), dim3(256),
              0, st, a);
    VR_HIP(hipGetLastError());
}

void launch_rows_gemm(const RowsGemmArgs& a, hipStream_t st, int tile) {
    VR_CHECK(rows_gemm_ok(a), -2, "rows_gemm: N, T, K, Cout >= 1, CoutPad >= Cout, a sample pitch of at least K T, at most 65535 cout tiles");
    if (!tile) tile = rows_gemm_tile(a);
    VR_CHECK(tile == 11 || tile == 21 || tile == 22, -2, "rows_gemm: tiles are 11 (16 couts x 16 positions), 21 (32 x 16) and 22 (32 x 32)");
    if (tile == 22) rows_gemm_launch<2, 2>(a, st);
    else if (tile == 21) rows_gemm_launch<2, 1>(a, st);
    else rows_gemm_launch<1, 1>(a, st);
}

}  // namespace vr
