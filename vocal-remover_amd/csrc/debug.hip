// Test hooks (tests/ only): single kernels of the training path behind vr_debug_kernel, host pointers in and out,
// so that every backward kernel has an isolated parity test against torch autograd (tests/test_gpu_kernels.py), the
// spectrogram-side glue of stft.hip against float64 numpy (tests/test_gpu_signal.py), and the LSTM fallbacks, the eval mask heads,
// the squeeze conv and the small kernels around them against oracle/kernel_refs.py (tests/test_gpu_heads_lstm.py), and ONE launch_conv in
// its general form -- concatenated strided sources, split strided destinations, a column window -- against oracle/kernel_refs.py
// (tests/test_gpu_conv_launch.py), and ONE launch_wgrad in its general form plus the two slab sums on synthetic slabs
// (tests/test_gpu_wgrad_launch.py), and ONE data gradient of a conv record (Model::bwd_conv_dgrad) in the network's forms
// (tests/test_gpu_dgrad_launch.py), and ONE launch_materialize, launch_upsample2x or launch_avgpool_h on a pending, strided tensor
// (tests/test_gpu_tensor_pass.py), and the derived weight forms those launches read -- one form of given weights through its single-layer and
// its batched launcher, and what a live handle holds for a layer (tests/test_gpu_weight_forms.py).
// The head_loss* and head_wave_* hooks run the train step's own head function (run_train_head, train.hip) on their buffers, and the
// wave_pair / wave_triple hooks the wave-term launcher it and vr_validate_step run (launch_wave_term, stft.hip): no copy of either here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "model.h"

namespace vr {

namespace {

struct DevBuf {
    float* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    explicit DevBuf(size_t n_) : n(n_) {
        VR_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(float)));
        // hipMemset on device memory returns before the fill has run, and the fill is on the NULL stream: the kernels of these hooks
        // run on the handle's non-blocking stream, which does not order against it -- wait here, or a late fill wipes a kernel's output
        // (seen once in round 5: test_gpu_hazard 'rows' victim off by whole values beside a busy aggressor)
        VR_HIP(hipMemset(p, 0, (n ? n : 1) * sizeof(float)));
        VR_HIP(hipStreamSynchronize(nullptr));
    }
    DevBuf(const float* host, size_t n_) : n(n_) {
        VR_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(float)));
        if (host && n) VR_HIP(hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice));
    }
    ~DevBuf() { if (p) hipFree(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    void download(float* host) const { if (host && n) VR_HIP(hipMemcpy(host, p, n * sizeof(float), hipMemcpyDeviceToHost)); }
};

Tensor dense(float* p, int N, int C, int H, int W) {
    Tensor t;
    t.p = p; t.N = N; t.C = C; t.H = H; t.W = W;
    t.sH = W; t.sC = (long long)H * W; t.sN = t.sC * C; t.slope = 1.f;
    return t;
}

// A host buffer uploaded as given between two guard bands, so that a store a little outside it lands in memory of the hook's own and is
// reported (intact()) instead of corrupting a neighbour's.  The bands are GUARD floats wide: a store further out is neither caught nor seen.
struct GuardedBuf {
    static constexpr size_t GUARD = 64;                   // floats: keeps p() 256-byte aligned
    static constexpr uint32_t PATTERN = 0x7fc5a5a5u;      // a quiet NaN no kernel produces
    DevBuf d;
    size_t n;
    GuardedBuf(const float* host, size_t n_) : d(n_ + 2 * GUARD), n(n_) {
        const std::vector<uint32_t> g(GUARD, PATTERN);
        VR_HIP(hipMemcpy(d.p, g.data(), GUARD * 4, hipMemcpyHostToDevice));
        VR_HIP(hipMemcpy(d.p + GUARD + n, g.data(), GUARD * 4, hipMemcpyHostToDevice));
        if (host && n) VR_HIP(hipMemcpy(p(), host, n * 4, hipMemcpyHostToDevice));
    }
    float* p() const { return d.p + GUARD; }
    void download(float* host) const { if (host && n) VR_HIP(hipMemcpy(host, p(), n * 4, hipMemcpyDeviceToHost)); }
    bool intact() const {
        std::vector<uint32_t> g(2 * GUARD);
        VR_HIP(hipMemcpy(g.data(), d.p, GUARD * 4, hipMemcpyDeviceToHost));
        VR_HIP(hipMemcpy(g.data() + GUARD, d.p + GUARD + n, GUARD * 4, hipMemcpyDeviceToHost));
        for (uint32_t v : g) if (v != PATTERN) return false;
        return true;
    }
};

// the strided view [N][C][H][W] at `off` lies inside a buffer of n floats
bool view_fits(long long off, long long sN, long long sC, long long sH, int N, int C, int H, int W, size_t n) {
    if (off < 0 || sN < 0 || sC < 0 || sH < 0 || N < 1 || C < 1 || H < 1 || W < 1) return false;
    return off + (N - 1) * sN + (C - 1) * sC + (H - 1) * sH + W <= (long long)n;
}

}  // namespace

ConvSrc make_src(const Tensor& t, bool up, int bcastH);   // model.hip
int wgrad_choose(WgradArgs& a, const ConvShape& s, int* CB, int* MT);      // wgrad_mfma.hip: the plan launch_wgrad launches

// name            dims                  fparams          inputs                                              outputs
// bn_backward     N,C,H,W[,floats,off,  slope,eps,mom    z, G, gamma, beta, post[N][C]|null, rm[C], rv[C]    dz, dgamma, dbeta, affine[C][2], rm, rv
//                 sN,sC,sH,aff_bcast]
//                 with the six trailing dims z and G are the view (off, sN, sC, sH) of two backing buffers of `floats` floats each (a conv
//                 output that is a channel slice of a wider buffer), given and returned whole, G between guard bands (error -3);
//                 aff_bcast 1 (C == 1): the affine table is the broadcast copy of the squeeze BatchNorm(1), BnBwdArgs::aff_bcast
// lstm            N,T,H[,flags]         -                gx[N][8H][T], whh_f[4H][H], whh_r, dh[N][2H][T]     h[N][2H][T], dgx[N][8H][T], dwhh_f, dwhh_r
//                                                        [, dwhh_f0[4H][H]|null, dwhh_r0|null]
//                 the W_hh gradient is ACCUMULATED onto dwhh_f0 / dwhh_r0 (zeros when absent).  flags bit 0: the inference form,
//                 launch_bilstm without a save buffer -- only h is produced, dh and the other outputs may be null; bit 1: only
//                 launch_bilstm_bwd, on a zeroed save buffer (its own size check, which the forward's would otherwise pre-empt)
// upsample        N,C,H,W[,floats,off,  -                x[N,C,H,W], dhi[N,C,2H,2W][, glo's backing buffer]  up[N,C,2H,2W], glo[N,C,H,W]
//                 sN,sC,sH,accumulate]
// pool            N,C,H,W[,floats,off,  -                x, gp[N,C,W], d[N,C,H,W][, g's backing buffer]      pooled[N,C,W], g[N,C,H,W], sumh[N,C,W]
//                 sN,sC,sH,accumulate]
//                 upsample / pool with the six trailing dims: the low-resolution gradient of launch_upsample_bwd / the gradient of
//                 launch_avgpool_bwd is the view (off, sN, sC, sH) of a backing buffer of `floats` floats, uploaded AS GIVEN (prior
//                 contents, canaries) between guard bands and returned whole in its output; accumulate 0 stores, 1 adds.  Without them:
//                 dense, accumulated onto zeros
// thin            N,C,H,W,CO            slope            x, aff[C][2]|null, w[CO][C], dz[N,CO,H,W]           g[N,C,H,W], dw[CO][C], z[N,H,W] (CO=1: forward)
// stft_crops      W,E,max_T,            -                wave w: float32 [2][n_w] (fmt 0) or its                rows [E][max_T][2][bins] complex64: entry e's
//                 W x (n,fmt,channels), interleaved sample bytes (padded to whole floats)     T_e rows at [e][0 .. T_e), zeros behind them
//                 E x (wave,start,T)
//                 launch 1 of a wave store's batch alone (launch_stft_crops, stft.hip): entry e = rows [start, start + T) of the STFT of
//                 wave `wave` at the handle's n_fft (hop == n_fft / 2), the scratch between guard bands (error -3).  fmt: 0 or a
//                 vr_pcm_format with its channel count; start >= 0, start + T <= 1 + n / hop and T <= max_T are checked here, as the
//                 entry points check them
// head_loss       N,C,H,W,bins          slope,gscale     x, aff|null, w[2][C], X[N,2,bins,W], Y              dlogit[N,2,H,W], mask[N,2,bins,W], loss[1]
// head_loss_complex N,C,H,W,bins        slope,gscale     x, aff|null, w[4][C], X[N,2,bins,W] complex64, Y    dlogit[N,4,H,W], mask[N,2,bins,W] complex64, loss[1],
//                                                        (complex64)                                         g[N,C,H,W], dw[4][C]
//                 run_train_head, the function Model::train_fwd_bwd_api runs, in its complex L1 form (loss = mean |m X - y| over the
//                 N*2*bins*W complex elements; then the CO = 4 thin weight and data gradients of that dlogit, both storing); head_loss
//                 is its real form without the thin gradients
// head            N,C,H,W,w_lo,w_hi,pad_rows,cplx,hsplit,use_items,pitch_extra
//                                       slope            x[N,C,H,W], aff0[C][2]|null, aff1[C][2]|null,       the destination(s), whole: dense [N][2][H+pad_rows][Wm +
//                                                        w[CO][C] (CO = 2; cplx: 4)                          pitch_extra], or with use_items one buffer per item n,
//                                                                                                            [2][H+pad_rows][Wm + pitch_extra + n] (cplx: complex64)
//                 launch_head_sigmoid / launch_head_complex; Wm = w_hi - w_lo; rows < hsplit take aff0, the others aff1; every
//                 destination is filled with NaN before the launch
// squeeze         N,C,H,W,use_part      slope            x, aff[C][2]|null, w[C], epi[2]|null                z[N,H,W], part[nblk][2]|null, nblk[1]|null
//                 launch_squeeze_conv; nblk = what its dry run returns
// head_bwd        N,H,W,bins            -                dmask[N,2,bins,W], mask[N,2,bins,W]                 dlogit[N,2,H,W]
// crop            rows,T,Wm,off,cplx    -                m[rows][Wm], x[rows][T], y[rows][T]|null            m * x[.., off + w] [rows][Wm], mean |that - y[.., off + w]|
//                 launch_mul_crop, launch_l1_crop (its real form only); cplx: m and x complex64, the complex product     [1]|null
// rows            N,R,W                 -                x[N,R,W], aff[R][2], d[N,R,W]                       relu(x*a+b), channel sums of d [R]
// adam            n                     lr,b1,b2,eps,gscale,step   p, g, m, v                                p, m, v
// wire            n                     -                x[n]                                                bf16_to_f32(f32_to_bf16(x)) [n]
// signal_norm     bins,T,Wpad,pad_l,mode,cplx   -        spec[2][bins][T] complex64                          mag_pad[2][bins][Wpad] (cplx: the packed planes
//                                                                                                            [4][bins][Wpad] of X / c), aff[4] (cplx: 1 / c in
//                                                                                                            aff[0..1]), sel[4] = the stats header as words:
//                                                                                                            max |X| bits, 0, key imag, key real (ord32 keys)
//                 mag_pad + coef_affine (cplx: mag_pad + coef_complex + pack_complex) as Model::separate runs them; mode 0 = max |X|,
//                 1 = numpy's lexicographic complex maximum of the zero-padded array
// signal_mask     T,Wa,Wb,shift,has_b,has_wgt,cplx   -   spec[2][bins][T] complex64, mask_a[2 bins][Wa],     fmin[T], y, v [2][bins][T] complex64,
//                                                        mask_b[2 bins][Wb]|null, wgt[T]|null                y_wave, v_wave [2][hop (T-1)] (fused masked
//                                                        (cplx: complex64 masks)                             iSTFT; hop == n_fft / 2 handles only)
//                 bins = n_fft / 2 + 1 of the handle; frame_min (no wgt), apply_mask and the masked iSTFT with `which` 0 and 1
// stream_post     T,RW,cut...           -                fmin[T]                                             weight[T], final_after[cuts + 1] (counts as floats),
//                                                                                                            ring[RW] as the last step left it
//                 The walk a VR_STREAM_POSTPROCESS stream runs (the rows == 0 form of frame_min_kernel's stream instantiation, stream_post.h's
//                 code on the device) on given minima, in steps: step k ends in front of frame cut[k] (ascending, in
//                 (0, T]), one more takes the rest and flushes.  Per step the minima are placed in a ring of RW entries (RW 0: 161 + the
//                 largest step, the least that works), a StreamSeg table of one entry is sent and the walk launched; a frame's weight is
//                 read back from the weight ring when it is declared final (below cut - 161; at the flush all), as
//                 vr_debug_stream_post_weight does on the host.  Both rings sit between guard bands (error -3).
// wave_eval       T,Wa,Wb,shift,has_b,  -                spec, mask_a, mask_b|null, wgt|null as signal_mask,  y_wave, v_wave [2][hop (T-1)] (store 0: left as they were
//                 has_wgt,cplx,window,                   mix[2][L], inst[2][L]                               allocated, zero), sums[windows][4] float64 (in a float32
//                 store,L                                                                                    buffer of twice the count), info[2] = (S, windows)
//                 One launch pair (which 0 and 1) of the evaluation form of istft_tile_kernel on a song table of one song, then
//                 launch_eval_sums (kernels.h: WaveEval): the stems signal_mask's fused masked iSTFT gives, and per
//                 window sum r_y^2, sum (r_y - y)^2, sum r_v^2, sum (r_v - v)^2 with r_y = inst, r_v = mix - inst.  window >= hop,
//                 L >= hop (T-1), T >= 2; S = the tile step (segments per workgroup).  Stems, partials and sums sit between guard bands
//                 (error -3).
// wave_pair       S,T,x_pitch,y_pitch,  -                x[S][bins][x_pitch] complex64, mask (same shape)    y_wave, p_wave [S][hop (T-1)], sums[3] = <y, p>,
//                 y_off,has_mask                         |null, y[S][bins][y_pitch] complex64                <y, y>, <p, p> over all signals
//                 launch_wave_term on a WavePair (launch_istft_pair + the launch_reduce_rows of its partials): the waves of the target y (frame t at column y_off + t) and
//                 of the estimate p = mask * x (no mask: x itself); bins = n_fft / 2 + 1 of the handle (hop == n_fft / 2 only).  Waves
//                 and partials sit between guard bands (error -3).
// wave_grad       S,T,l1                sdr_scale,       y_wave, p_wave [S][hop (T-1)], sums[3], X[S][bins]  dmask[S][bins][T] complex64
//                                       l1_scale         [T] complex64, mask|null, Y|null (same shape)
//                 launch_stft_wave_grad (kernels.h: WaveGrad); l1 0 switches the magnitude-L1 part off (mask and Y are then not read);
//                 dmask sits between guard bands (error -3)
// head_wave_loss  N,C,H,W,bins[,       slope,sdr_scale, x, aff|null, w[4][C], X[N,2,bins,W] complex64, Y    dlogit[N,4,H,W], mask[N,2,bins,W] complex64, loss[4] =
//                 head_only]            l1_scale                                                             (mean ||y|-|p||, <y,p>, <y,y>, <p,p>), g[N,C,H,W],
//                                                                                                            dw[4][C], dmask[N,2,bins,W] complex64
//                 run_train_head in its VR_LOSS_MAG_L1_WAVE_SDR form, the call Model::train_fwd_bwd_api makes: launch_head_mag_l1, the pair
//                 wave term, launch_stft_wave_grad, launch_head_bwd_complex, then the CO = 4 thin gradients (storing); bins = n_fft / 2 + 1
//                 of the handle, W = the frames.  A sixth dim head_only = 1: the same call without gradient destinations, which stops
//                 after launch_head_mag_l1, at any bins >= H -- only mask and loss[0] are produced
// wave_triple     S,T,xy_pitch,xy_off,  -                x, y [S][bins][xy_pitch] complex64, mask (same      x_wave, y_wave, p_wave [S][hop (T-1)], sums[6] = <y, p>,
//                 p_pitch,has_mask                       shape)|null, p[S][bins][p_pitch] complex64|null     <y, y>, <p, p>, <n, q>, <n, n>, <q, q> over all signals
//                 launch_wave_term on a WaveTriple (launch_istft_triple + the launch_reduce_rows of its partials; kernels.h: WaveTriple): the waves of
//                 the mixture x and the target y (frame t at column xy_off + t) and of the estimate -- mask * x with a mask, else p (frame t
//                 at column t); n = x_wave - y_wave, q = x_wave - p_wave.  Waves and partials sit between guard bands (error -3).
// wave_grad3      S,T,l1                sdr_scale,       x_wave, y_wave, p_wave [S][hop (T-1)], sums[6],     dmask[S][bins][T] complex64
//                                       l1_scale         X[S][bins][T] complex64, mask|null, Y|null
//                 launch_stft_wave_grad3 (kernels.h: WaveGrad3); l1 as for wave_grad; dmask sits between guard bands (error -3)
// head_wave_wsdr  N,C,H,W,bins          slope,sdr_scale, x, aff|null, w[4][C], X[N,2,bins,W] complex64, Y    dlogit[N,4,H,W], mask[N,2,bins,W] complex64, loss[7] =
//                                       l1_scale                                                             (mean ||y|-|p||, the six sums), g[N,C,H,W],
//                                                                                                            dw[4][C], dmask[N,2,bins,W] complex64
//                 run_train_head in its VR_LOSS_MAG_L1_WAVE_WSDR form, the call Model::train_fwd_bwd_api makes: launch_head_mag_l1, the triple
//                 wave term, launch_stft_wave_grad3, launch_head_bwd_complex, then the CO = 4 thin gradients (storing); bins = n_fft / 2 + 1
//                 of the handle, W = the frames.  Waves, partials and dmask sit between guard bands (error -3).
// conv_launch     nsrc,ndst,N,Cout,KS,  epi_slope,       w[Cout][Cin][KS][KS] (OIHW), bias[Cout]|null,       per destination its whole backing buffer (null where
//                 dil_h,dil_w,flags,    slope of         epi[Cout][2]|null; per source: its backing buffer,  absent); then, with flags bit 1, stats[Cout][2] =
//                 w_lo,w_hi,d1,d2;      source 0, 1, 2   aff0[C][2]|null, aff1[C][2]|null, post[N][C]|null;   the BatchNorm partials summed per channel
//                 per source C,H,W,up,                   per destination its backing buffer, uploaded AS
//                 hsplit,floats,off,                     GIVEN (null where absent)
//                 sN,sC,sH; per
//                 destination present,
//                 accumulate,floats,
//                 off,sN,sC,sH
//                 ONE launch_conv (stride 1, 'same' padding) in its general form, on the handle's stream and in its mfma_mode.  A source is
//                 the view (off, sN, sC, sH) of its backing buffer of `floats` floats (C, H, W before the x2 upsample `up`), a destination
//                 the view of its own; output channels [0, d1) go to destination 0, [d1, d2) to 1, the others to 2.  flags bit 0: the
//                 transformed weight forms of the mode (as vr_debug_conv2d's bit 1), bit 1: partials.  Error -2: a view that leaves its
//                 buffer, and every refusal of launch_conv (message intact).  Error -3: a store found in the 64 floats in front of or
//                 behind a destination's buffer (the guard bands; a store further out is not seen).
// wgrad_launch    nsrc,N,Cout,KS,stride, slope of         dz's backing buffer, the gradient buffer            the gradient buffer, whole, as the device left it;
//                 dil_h,dil_w,flags,    source 0, 1, 2   [Cin][KS*KS][CoutPad] uploaded AS GIVEN (prior       info = four int64 in eight floats: P (the plan's slab
//                 dz floats,off,sN,sC,                   contents and canaries are the caller's); per        count), part_stride, the scratch floats, the
//                 sH; per source C,H,W,                  source: its backing buffer, aff0[C][2]|null,        descriptors the deferred sum took
//                 up,hsplit,floats,off,                  aff1[C][2]|null, post[N][C]|null
//                 sN,sC,sH
//                 ONE launch_wgrad in its general form, on the handle's stream, in its mfma_mode and train_winograd (allow_wino).  Sources
//                 as conv_launch has them; dz is the view (off, sN, sC, sH) [N][Cout][Hout][Wout] of its buffer.  flags bit 0: batch_as_h
//                 (1x1 on H = 1: build_fwd_args' rewrite of the sources and bwd_conv's of zN / zH), bit 1: accumulate, bit 2: defer (the
//                 sink set as Model::backward sets it, then flush_wgrad_sums()), bit 3: the launch is issued a second time under the same
//                 sink, into the same gradient from a scratch slab of its own, accumulating if bit 4 is set.  The scratch slab is sized
//                 by wgrad_scratch_floats and filled with NaN; gradient and scratch sit between guard bands.  P and part_stride are those
//                 of wgrad_choose, the function launch_wgrad itself takes its plan from, on the same arguments.  Error -2: a view that leaves
//                 its buffer, and every refusal of launch_wgrad (message intact).  Error -3: a store found in a guard band.
// dgrad_launch    nsrc,N,Cout,KS,stride, -               w[Cout][Cin][KS][KS] (OIHW), dz's backing buffer;   per source its gradient's backing buffer, whole, as
//                 dil_h,dil_w,flags,                     per source the backing buffer of its gradient,      the device left it; info = four int64 in eight
//                 dz floats,off,sN,sC,                   uploaded AS GIVEN (prior contents and canaries      floats: the path (Model::DgradPath: 1 stride 1,
//                 sH; per source C,H,W,                  are the caller's)                                   2 fused parity classes, 3 four tap-masked launches,
//                 up,bcastH,mode,floats,                                                                     4 zero insertion), the workspace floats, 0, 0
//                 off,sN,sC,sH
//                 ONE Model::bwd_conv_dgrad: the data gradient of a conv record and the passes after it (launch_upsample_bwd for an `up`
//                 source, launch_sum_h for a `bcastH` one), on the handle's stream, in its mfma_mode and train_winograd, with the
//                 transposed weight forms a train step would hold (Model::debug_dgrad_weight_forms).  dz is the view (off, sN, sC, sH)
//                 [N][Cout][Hout][Wout] of its buffer; a source's gradient the view [N][C][H][W] of its own (C, H, W before the x2
//                 upsample `up`; H = 1 with bcastH = the rows it is broadcast over, and then dense: launch_sum_h takes no strides).  mode 0:
//                 the source takes no gradient (its buffer must come back untouched), 1: the first writer stores (the hook marks the
//                 buffer fresh, Model::g_fresh), 2: accumulate.  flags bit 0: batch_as_h.  The workspace is sized by a dry pass, filled
//                 with NaN, and like every gradient buffer sits between guard bands.  Error -2: a view that leaves its buffer and every
//                 refusal of a launch (message intact; the outputs then hold the buffers as the refused call left them).  Error -3: a
//                 store found in a guard band.
// wgrad_reduce    nd; per descriptor    -                per descriptor: its slabs [P][stride], its output   per descriptor: its output buffer after
//                 P,n,stride,                            buffer (prior contents) of `floats` floats          wgrad_reduce_kernel, the same after the batched sum;
//                 accumulate,floats,off                                                                      then vec[1] = what wgrad_reduce_vec chose
//                 The two slab sums on synthetic slabs: every descriptor once through launch_wgrad_reduce, one by one, and all of them once
//                 through wred_host + flush_wgrad_sums().  A descriptor sums into the n floats at `off` of its output buffer.
// tensor_pass     op,N,C,H,W,floats,off, slope            the source's backing buffer, aff0[C][2]|null,       the result, dense and whole (null with inplace); the
//                 sN,sC,sH,hsplit,                       aff1[C][2]|null, post[N][C]|null                    source's backing buffer as the device left it
//                 bcastH,inplace
//                 ONE pass over a pending tensor, on the handle's stream: the view (off, sN, sC, sH) [N][C][H][W] of a backing buffer of
//                 `floats` floats, uploaded AS GIVEN, with its affines (rows < hsplit take aff0, the others aff1), slope and multiplier.
//                 op 0: launch_materialize -> [N][C][Hv][W]; with bcastH > 0 the source has H == 1 and the launch gets H = bcastH, sH = 0,
//                 as Model::run_conv forms it (Hv = bcastH, else H).  op 1: launch_upsample2x -> [N][C][2H][2W].  op 2: launch_avgpool_h
//                 -> [N][C][W].  The result buffer is 16-byte aligned, filled with the NaN canary 0x7FC12345 and, like the source's, sits
//                 between guard bands.  inplace 1 (op 0, a dense view at off 0, no bcastH): the launch writes onto the source itself, as
//                 Model::separate does; the result is then the returned source buffer.  Error -2: a view that leaves its buffer, and
//                 every refusal of a launcher (message intact; the outputs then hold the buffers as the refused call left them).
//                 Error -3: a store found in a guard band.
// weight_forms    form,nd; per           -                per descriptor: w[Cout][Cin][KS][KS] (OIHW)         per descriptor: the form's buffer, whole, as float32
//                 descriptor Cin,Cout,KK                                                                     words, after the single-layer launcher (null: skipped),
//                                                                                                            then the same after the batched launch
//                 ONE derived weight form (0 wino, 1 wino6, 2 x3, 3 x3h, 4 flip, 5 s2_class; oracle/kernel_refs.py states each) of nd
//                 layers, from their K-major copies [Cin][KK][CoutPad] with zeroed padded couts, on the handle's stream: once per
//                 descriptor through launch_wino_weights / launch_wino_weights6 / launch_x3_weights / launch_x3h_weights (flip and
//                 s2_class exist only in batched form: a table of one descriptor), and once for all descriptors in ONE launch of the
//                 batched launcher, its grid sized as Model::fill_form sizes it.  Every buffer has
//                 the size the library gives it (x3_weights_bytes, wino_weights6_bytes, Cin 16 CoutPad, Cout KK CinPad, 4 Cout 9
//                 CinPad), is filled with the NaN canary 0x7FC12345 and sits between guard bands.  Error -3: a store found in a guard band.
// layer_forms     i[,capacity]           -                -                                                   i = -1: out[0] = the layer count, then per conv in
//                                                                                                            for_each_conv's order Cin, Cout, KS, stride, dh, dw,
//                                                                                                            mask (`capacity` floats); else the K-major weights
//                                                                                                            [Cin][KK][CoutPad], then the buffers of the mask
//                 What the handle holds for conv i, read-only, after the handle's stream has drained.  Mask bits and outputs 1..9 in this
//                 order: wino [Cin][16][CoutPad], wino6, x3w (x3_weights_bytes of Cin, KK, CoutPad), wt [Cout][KK][CinPad], winot
//                 [Cout][16][CinPad], winot6, x3t and x3dt (x3_weights_bytes of Cout, KK, CinPad), s2w [4][Cout][9][CinPad].  A
//                 null output is skipped; an output for a buffer the handle does not hold is error -2.  A set bit says that the buffer
//                 exists, not that the current mfma_mode fills it.  The buffers are the slots of the conv's record (Conv::forms,
//                 weight_forms.h) and their sizes come from form_spec, the rule the handle allocates by: a new form is added there.
//                 The record has ONE slot for the planes of wt; it is reported as x3t for a plain 3x3, as x3dt for a conv_x3d layer.
namespace {

constexpr uint32_t FORM_CANARY = 0x7fc12345u;

template <class D>
struct DevTable {                                         // a descriptor table of a batched launch
    D* p = nullptr;
    explicit DevTable(const std::vector<D>& v) {
        VR_HIP(hipMalloc(reinterpret_cast<void**>(&p), v.size() * sizeof(D)));
        VR_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(D), hipMemcpyHostToDevice));
    }
    ~DevTable() { (void)hipFree(p); }
    DevTable(const DevTable&) = delete;
    DevTable& operator=(const DevTable&) = delete;
};

int round32(int v) { return (v + 31) / 32 * 32; }

}  // namespace

void Model::debug_weight_form_launch(const int64_t* dims, int ndims, const float* const* in, int nin, float* const* out, int nout) {
    const std::string who = "vr_debug_kernel(weight_forms): ";
    VR_CHECK(ndims >= 2, -2, who + "too few arguments");
    const int form = (int)dims[0], nd = (int)dims[1];
    VR_CHECK(form >= 0 && form <= 5 && nd >= 1 && nd <= 64 && ndims >= 2 + 3 * nd && nin >= nd && nout >= 2 * nd, -2,
             who + "form 0..5, 1..64 descriptors of three dims each, two outputs per descriptor");
    std::vector<std::unique_ptr<DevBuf>> wk;
    std::vector<std::unique_ptr<GuardedBuf>> one, bat;
    std::vector<WinoWDesc> wd;
    std::vector<X3WDesc> xd;
    std::vector<FlipDesc> fd;
    std::vector<S2WDesc> sd;
    for (int j = 0; j < nd; ++j) {
        const int Cin = (int)dims[2 + 3 * j], Cout = (int)dims[3 + 3 * j], KK = (int)dims[4 + 3 * j];
        VR_CHECK(Cin >= 1 && Cin <= 4096 && Cout >= 1 && Cout <= 4096 && (KK == 9 || (KK == 1 && (form == 2 || form == 3 || form == 4))), -2,
                 who + "1..4096 channels; KK is 9, or 1 for x3, x3h and flip");
        VR_CHECK(in[j] && out[nd + j], -2, who + "a descriptor needs its weights and its batched output");
        const int CoutPad = round32(Cout), CinPad = round32(Cin);
        std::vector<float> h((size_t)Cin * KK * CoutPad, 0.f);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < Cin; ++ci)
                for (int k = 0; k < KK; ++k) h[((size_t)ci * KK + k) * CoutPad + co] = in[j][((size_t)co * Cin + ci) * KK + k];
        wk.emplace_back(new DevBuf(h.data(), h.size()));
        const float* w = wk.back()->p;
        const size_t words = form == 0 ? (size_t)Cin * 16 * CoutPad
                           : form == 1 ? wino_weights6_bytes(Cin, CoutPad) / 4
                           : form <= 3 ? x3_weights_bytes(Cin, KK, CoutPad) / 4
                           : form == 4 ? (size_t)Cout * KK * CinPad : (size_t)4 * Cout * 9 * CinPad;
        const std::vector<uint32_t> canary(words, FORM_CANARY);
        one.emplace_back(new GuardedBuf(reinterpret_cast<const float*>(canary.data()), words));
        bat.emplace_back(new GuardedBuf(reinterpret_cast<const float*>(canary.data()), words));
        float* o1 = one.back()->p();
        float* ob = bat.back()->p();
        switch (form) {
        case 0: launch_wino_weights(w, o1, Cin, CoutPad, stream); wd.push_back(WinoWDesc{w, ob, Cin, CoutPad}); break;
        case 1: launch_wino_weights6(w, o1, Cin, CoutPad, stream); wd.push_back(WinoWDesc{w, ob, Cin, CoutPad}); break;
        case 2: launch_x3_weights(w, o1, Cin, KK, CoutPad, stream); xd.push_back(X3WDesc{w, ob, Cin, KK, CoutPad}); break;
        case 3: launch_x3h_weights(w, o1, Cin, KK, CoutPad, stream); xd.push_back(X3WDesc{w, ob, Cin, KK, CoutPad}); break;
        case 4: {
            const std::vector<FlipDesc> t{FlipDesc{w, o1, Cin, Cout, KK, CinPad, CoutPad}};
            DevTable<FlipDesc> dt(t);
            launch_flip_transpose(dt.p, 1, stream);
            VR_HIP(hipStreamSynchronize(stream));             // (the table is freed at the brace)
            fd.push_back(FlipDesc{w, ob, Cin, Cout, KK, CinPad, CoutPad});
            break;
        }
        default: {
            const std::vector<S2WDesc> t{S2WDesc{w, o1, Cin, Cout, CoutPad, CinPad}};
            DevTable<S2WDesc> dt(t);
            launch_s2_class_weights(dt.p, 1, s2w_batch_max_elems(t), stream);
            VR_HIP(hipStreamSynchronize(stream));
            sd.push_back(S2WDesc{w, ob, Cin, Cout, CoutPad, CinPad});
            break;
        }
        }
    }
    // all descriptors in ONE launch of the batched launcher
    if (form <= 1) {
        DevTable<WinoWDesc> dt(wd);
        launch_wino_weights_batched(dt.p, nd, wino_batch_max_elems(wd, form == 1), form == 1, stream);
        VR_HIP(hipStreamSynchronize(stream));
    } else if (form <= 3) {
        DevTable<X3WDesc> dt(xd);
        if (form == 3) launch_x3h_weights_batched(dt.p, nd, x3_batch_max_elems(xd), x3_batch_max_cout_pad(xd), stream);
        else launch_x3_weights_batched(dt.p, nd, x3_batch_max_elems(xd), stream);
        VR_HIP(hipStreamSynchronize(stream));
    } else if (form == 4) {
        DevTable<FlipDesc> dt(fd);
        launch_flip_transpose(dt.p, nd, stream);
        VR_HIP(hipStreamSynchronize(stream));
    } else {
        DevTable<S2WDesc> dt(sd);
        launch_s2_class_weights(dt.p, nd, s2w_batch_max_elems(sd), stream);
        VR_HIP(hipStreamSynchronize(stream));
    }
    for (int j = 0; j < nd; ++j) VR_CHECK(one[j]->intact() && bat[j]->intact(), -3, who + "a launch stored outside its form's buffer");
    for (int j = 0; j < nd; ++j) {
        one[j]->download(out[j]);
        bat[j]->download(out[nd + j]);
    }
}

void Model::debug_layer_forms(const int64_t* dims, int ndims, float* const* out, int nout) {
    const std::string who = "vr_debug_kernel(layer_forms): ";
    VR_CHECK(ndims >= 1 && nout >= 1 && out[0], -2, who + "too few arguments");
    VR_HIP(hipStreamSynchronize(stream));
    const std::vector<Conv*> convs = conv_layers();
    static const FormId form_of[9] = {F_WINO, F_WINO6, F_X3W, F_WT, F_WINOT, F_WINOT6, F_X3T, F_X3T, F_S2W};
    auto held = [&](const Conv& L, void* b[9]) {
        for (int j = 0; j < 9; ++j) b[j] = L.forms.p[form_of[j]];
        b[L.cls == FC_X3D ? 6 : 7] = nullptr;
    };
    const long long i = dims[0];
    if (i < 0) {
        VR_CHECK(ndims >= 2 && dims[1] >= (long long)(1 + 7 * convs.size()), -2, who + "the table needs 1 + 7 floats per conv");
        out[0][0] = (float)convs.size();
        for (size_t k = 0; k < convs.size(); ++k) {
            const Conv& L = *convs[k];
            void* b[9];
            held(L, b);
            int mask = 0;
            for (int j = 0; j < 9; ++j) mask |= b[j] ? 1 << j : 0;
            const int row[7] = {L.Cin, L.Cout, L.KS, L.stride, L.dh, L.dw, mask};
            for (int j = 0; j < 7; ++j) out[0][1 + 7 * k + j] = (float)row[j];
        }
        return;
    }
    VR_CHECK(i < (long long)convs.size() && nout >= 10, -2, who + "no such conv, or fewer than ten outputs");
    const Conv& L = *convs[(size_t)i];
    void* b[9];
    held(L, b);
    VR_HIP(hipMemcpy(out[0], L.w->dev, (size_t)L.Cin * L.KS * L.KS * L.CoutPad * 4, hipMemcpyDeviceToHost));
    for (int j = 0; j < 9; ++j) {
        if (!out[1 + j]) continue;
        VR_CHECK(b[j], -2, who + "the handle holds no such buffer for this conv");
        VR_HIP(hipMemcpy(out[1 + j], b[j], form_spec(form_of[j], L, mfma_mode, W6_PAD64).bytes, hipMemcpyDeviceToHost));
    }
}

void Model::debug_tensor_pass(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                              int nout) {
    const std::string who = "vr_debug_kernel(tensor_pass): ";
    VR_CHECK(ndims >= 13 && nfp >= 1 && nin >= 4 && nout >= 2, -2, who + "too few arguments");
    const int op = (int)dims[0], N = (int)dims[1], C = (int)dims[2], H = (int)dims[3], W = (int)dims[4];
    const long long floats = dims[5], off = dims[6], sN = dims[7], sC = dims[8], sH = dims[9];
    const int bcastH = (int)dims[11];
    const bool inplace = dims[12] != 0;
    VR_CHECK(op >= 0 && op <= 2 && bcastH >= 0 && floats >= 1 && floats <= (1LL << 28), -2, who + "op is 0, 1 or 2; bcastH >= 0");
    VR_CHECK(in[0] && out[1] && (inplace || out[0]), -2, who + "missing the source buffer or an output");
    VR_CHECK(view_fits(off, sN, sC, sH, N, C, H, W, (size_t)floats), -2, who + "the source view leaves its buffer");
    VR_CHECK(!bcastH || (op == 0 && H == 1), -2, who + "a broadcast source is materialised (op 0) and has H = 1");
    VR_CHECK(!inplace || (op == 0 && !bcastH && off == 0 && sH == W && sC == (long long)H * W && sN == sC * C), -2,
             who + "in place: op 0 on a dense view at off 0 without bcastH");
    const int Hv = bcastH ? bcastH : H;
    const size_t n = op == 0 ? (size_t)N * C * Hv * W : (op == 1 ? (size_t)4 * N * C * H * W : (size_t)N * C * W);
    VR_CHECK(n <= ((size_t)1 << 28), -2, who + "the result is too large for a test hook");
    GuardedBuf src(in[0], (size_t)floats);
    const std::vector<uint32_t> canary(inplace ? 0 : n, 0x7fc12345u);
    GuardedBuf res(inplace ? nullptr : reinterpret_cast<const float*>(canary.data()), inplace ? 0 : n);
    DevBuf aff0(in[1], in[1] ? (size_t)C * 2 : 0), aff1(in[2], in[2] ? (size_t)C * 2 : 0), post(in[3], in[3] ? (size_t)N * C : 0);
    Tensor t;
    t.p = src.p() + off; t.N = N; t.C = C; t.H = Hv; t.W = W;
    t.sN = sN; t.sC = sC; t.sH = bcastH ? 0 : sH;
    t.hsplit = (int)dims[10]; t.slope = fp[0];
    if (in[1]) t.aff0 = aff0.p;
    if (in[2]) t.aff1 = aff1.p;
    if (in[3]) t.post = post.p;
    float* dst = inplace ? t.p : res.p();
    try {
        if (op == 0) launch_materialize(t, dst, stream);
        else if (op == 1) launch_upsample2x(t, dst, stream);
        else launch_avgpool_h(t, dst, stream);
    } catch (...) {                                       // a refusal: the caller still sees what the buffers hold (nothing may have been written)
        (void)hipStreamSynchronize(stream);
        if (!inplace) res.download(out[0]);
        src.download(out[1]);
        throw;
    }
    VR_HIP(hipStreamSynchronize(stream));
    VR_CHECK(src.intact() && res.intact(), -3, who + "the launch stored outside the result or the source buffer");
    if (!inplace) res.download(out[0]);
    src.download(out[1]);
}

void Model::debug_conv_launch(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin,
                              float* const* out, int nout) {
    const std::string who = "vr_debug_kernel(conv_launch): ";
    VR_CHECK(ndims >= 12 && nfp >= 4, -2, who + "too few arguments");
    const int nsrc = (int)dims[0], ndst = (int)dims[1], N = (int)dims[2], Cout = (int)dims[3], KS = (int)dims[4];
    const int dh = (int)dims[5], dw = (int)dims[6], flags = (int)dims[7];
    const bool transformed = flags & 1, want_part = flags & 2;
    VR_CHECK(nsrc >= 1 && nsrc <= 3 && ndst >= 1 && ndst <= 3 && N >= 1 && Cout >= 1 && (KS == 1 || KS == 3) && dh >= 1 && dw >= 1, -2,
             who + "1..3 sources and destinations, a 1x1 or 3x3 kernel");
    VR_CHECK(ndims >= 12 + 10 * nsrc + 7 * ndst && nin >= 3 + 4 * nsrc + ndst && nout >= ndst + (want_part ? 1 : 0), -2,
             who + "too few arguments");
    VR_CHECK(in[0] && (!want_part || out[ndst]), -2, who + "missing weights or partials output");
    ConvArgs a{};
    a.nsrc = nsrc; a.N = N; a.Cout = Cout; a.CoutPad = (Cout + 31) / 32 * 32;
    a.w_lo = (int)dims[8]; a.w_hi = (int)dims[9]; a.d1 = (int)dims[10]; a.d2 = (int)dims[11];
    a.bf16 = mfma_mode;
    a.pad_h = KS == 1 ? 0 : dh; a.pad_w = KS == 1 ? 0 : dw;
    // sources
    std::vector<std::unique_ptr<DevBuf>> keep;
    auto upload = [&](const float* host, size_t n) { keep.emplace_back(new DevBuf(host, n)); return keep.back()->p; };
    int Cin = 0;
    const ConvSrc* ups = nullptr;
    for (int i = 0; i < nsrc; ++i) {
        const int64_t* d = dims + 12 + 10 * i;
        const float* const* si = in + 3 + 4 * i;
        Tensor t;
        t.N = N; t.C = (int)d[0]; t.H = (int)d[1]; t.W = (int)d[2];
        const bool up = d[3] != 0;
        t.hsplit = (int)d[4];
        const size_t floats = (size_t)d[5];
        t.sN = d[7]; t.sC = d[8]; t.sH = d[9];
        VR_CHECK(si[0] && view_fits(d[6], t.sN, t.sC, t.sH, N, t.C, t.H, t.W, floats), -2, who + "a source view leaves its buffer");
        t.p = upload(si[0], floats) + d[6];
        t.slope = fp[1 + i];
        if (si[1]) t.aff0 = upload(si[1], (size_t)t.C * 2);
        if (si[2]) t.aff1 = upload(si[2], (size_t)t.C * 2);
        if (si[3]) t.post = upload(si[3], (size_t)N * t.C);
        a.src[i] = make_src(t, up, 0);
        const int vh = up ? 2 * t.H : t.H, vw = up ? 2 * t.W : t.W;
        if (i == 0) { a.Hin = vh; a.Win = vw; }
        VR_CHECK(vh == a.Hin && vw == a.Win, -2, who + "the sources must share the input size");
        // (Model::build_fwd_args' rule: the loaders keep one interpolation table per workgroup)
        if (up && ups) VR_CHECK(ups->H == t.H && ups->W == t.W && ups->sH == t.sH, -2, who + "upsampled sources must share H, W and row stride");
        if (up) ups = &a.src[i];
        Cin += t.C;
        if (i == 0) a.c1 = Cin;
        if (i <= 1) a.c2 = Cin;                           // (a missing source is an empty channel range at the end)
    }
    a.Cin = Cin;
    a.Hout = a.Hin; a.Wout = a.Win;
    // weights: K-major [Cin][KS*KS][CoutPad], then the forms of the mode
    const int KK = KS * KS;
    std::vector<float> wk((size_t)Cin * KK * a.CoutPad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < KK; ++k) wk[((size_t)ci * KK + k) * a.CoutPad + co] = in[0][((size_t)co * Cin + ci) * KK + k];
    DevBuf dwk(wk.data(), wk.size());
    a.w = dwk.p;
    if (in[1]) a.bias = upload(in[1], (size_t)Cout);
    if (in[2]) { a.epi = upload(in[2], (size_t)Cout * 2); a.epi_slope = fp[0]; }
    LocalConv wf;
    debug_weight_forms(dwk.p, Cin, KS, 1, dh, dw, a.CoutPad, a.Win, transformed, a, wf);
    // destinations
    std::vector<std::unique_ptr<GuardedBuf>> dst(3);
    const int c1 = a.d1 < Cout ? a.d1 : Cout, c2 = a.d2 < Cout ? a.d2 : Cout;
    VR_CHECK(0 <= c1 && c1 <= c2, -2, who + "need 0 <= d1 <= d2");
    const int seg_c[3] = {c1, c2 - c1, Cout - c2};
    for (int i = 0; i < ndst; ++i) {
        const int64_t* d = dims + 12 + 10 * nsrc + 7 * i;
        const float* host = in[3 + 4 * nsrc + i];
        if (!d[0]) continue;                              // absent: p stays null
        VR_CHECK(host && out[i], -2, who + "a present destination needs its buffer, in and out");
        VR_CHECK(seg_c[i] == 0 || view_fits(d[3], d[4], d[5], d[6], N, seg_c[i], a.Hout, a.Wout, (size_t)d[2]), -2,
                 who + "a destination view leaves its buffer");
        dst[i].reset(new GuardedBuf(host, (size_t)d[2]));
        a.dst[i] = ConvDst{dst[i]->p() + d[3], d[4], d[5], d[6], d[1] != 0 ? 1 : 0, 0};
    }
    const ConvShape shp{KS, 1, dh, dw};
    size_t npt = 0;
    std::unique_ptr<DevBuf> part;
    if (want_part) { npt = conv_part_count(a, shp); part.reset(new DevBuf(npt * Cout * 2)); a.part = part->p; }
    launch_conv(a, shp, stream);
    VR_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < ndst; ++i)
        if (dst[i]) {
            VR_CHECK(dst[i]->intact(), -3, who + "the launch stored outside a destination's buffer");
            dst[i]->download(out[i]);
        }
    if (want_part) {
        std::vector<float> ph(npt * Cout * 2);
        part->download(ph.data());
        for (int c = 0; c < Cout; ++c) {
            double s1 = 0, s2 = 0;
            for (size_t i = 0; i < npt; ++i) { s1 += ph[(i * Cout + c) * 2]; s2 += ph[(i * Cout + c) * 2 + 1]; }
            out[ndst][2 * c] = (float)s1; out[ndst][2 * c + 1] = (float)s2;
        }
    }
}

// conv_tail       nsrc,N,Cout,kind,     slope of the     w1[Cout][Cin][3][3] (OIHW), epi1[Cout][2],          y's backing buffer, whole, as the device left it;
//                 Cout2,MT,TH,          3x3 stage, of    w2[Cout2][Cout], epi2[Cout2][2], y's backing        the 3x3 stage's output [N][Cout][H][W] (null: not
//                 y floats,off,sN,sC,   the 1x1 stage    buffer uploaded AS GIVEN; per source its            wanted; kind 1 fused: never written, returned as
//                 sH; per source C,H,W,                  backing buffer                                      the zeros it was allocated with)
//                 up,floats,off,sN,sC,sH
//                 A 3x3 conv + folded BatchNorm + activation on conv_x3h.hip in the tiling <MT, TH> (mfma_mode 3), and the 1x1 stage that
//                 reads its output: kind 1 a Conv2DBNActiv Cout -> Cout2 into the view (off, sN, sC, sH) of y (the stage tails of the
//                 low-band nets), kind 2 the LSTM squeeze Cout -> 1 + BatchNorm + ReLU into y [N][H][W].  With the handle's option
//                 fuse_tail on: ONE launch (ConvArgs::tail; refused, -2, where x3h_tail_ok refuses); off: the two launches of the
//                 executor (launch_conv's 1x1 / launch_squeeze_conv behind the same conv_x3h launch).  y sits between guard bands (-3).
void Model::debug_conv_tail(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                            int nout) {
    const std::string who = "vr_debug_kernel(conv_tail): ";
    VR_CHECK(ndims >= 12 && nfp >= 2 && nout >= 2, -2, who + "too few arguments");
    const int nsrc = (int)dims[0], N = (int)dims[1], Cout = (int)dims[2], kind = (int)dims[3], Cout2 = (int)dims[4];
    const ConvPlan tile{CK_X3, (int)dims[5], (int)dims[6], 32, nullptr};       // the tiling is the test's, not conv_plan's
    VR_CHECK(nsrc >= 1 && nsrc <= 3 && N >= 1 && Cout >= 1 && (kind == 1 || kind == 2) && Cout2 >= 1 && (kind == 1 || Cout2 == 1), -2,
             who + "1..3 sources, kind 1 or 2");
    VR_CHECK((tile.MT == 32 || tile.MT == 64) && (tile.TH == 8 || (tile.TH == 16 && tile.MT == 32)), -2, who + "tilings: <32,8>, <32,16>, <64,8>");
    VR_CHECK(mfma_mode == 3, -2, who + "conv_x3h runs in mfma_mode 3");
    VR_CHECK(ndims >= 12 + 9 * nsrc && nin >= 5 + nsrc && in[0] && in[1] && in[2] && in[3] && in[4] && out[0], -2, who + "too few arguments");
    ConvArgs a{};
    a.nsrc = nsrc; a.N = N; a.Cout = Cout; a.CoutPad = (Cout + 31) / 32 * 32;
    VR_CHECK(a.CoutPad % tile.MT == 0, -2, who + "the cout tile does not divide the padded couts");
    a.d1 = a.d2 = 1 << 30;
    a.bf16 = 3;
    a.pad_h = a.pad_w = 1;
    std::vector<std::unique_ptr<DevBuf>> keep;
    auto upload = [&](const float* host, size_t n) { keep.emplace_back(new DevBuf(host, n)); return keep.back()->p; };
    int Cin = 0;
    const ConvSrc* ups = nullptr;
    for (int i = 0; i < nsrc; ++i) {
        const int64_t* d = dims + 12 + 9 * i;
        Tensor t;
        t.N = N; t.C = (int)d[0]; t.H = (int)d[1]; t.W = (int)d[2];
        const bool up = d[3] != 0;
        const size_t floats = (size_t)d[4];
        t.sN = d[6]; t.sC = d[7]; t.sH = d[8];
        VR_CHECK(in[5 + i] && view_fits(d[5], t.sN, t.sC, t.sH, N, t.C, t.H, t.W, floats), -2, who + "a source view leaves its buffer");
        t.p = upload(in[5 + i], floats) + d[5];
        t.slope = 1.f;
        a.src[i] = make_src(t, up, 0);
        const int vh = up ? 2 * t.H : t.H, vw = up ? 2 * t.W : t.W;
        if (i == 0) { a.Hin = vh; a.Win = vw; }
        VR_CHECK(vh == a.Hin && vw == a.Win, -2, who + "the sources must share the input size");
        if (up && ups) VR_CHECK(ups->H == t.H && ups->W == t.W && ups->sH == t.sH, -2, who + "upsampled sources must share H, W and row stride");
        if (up) ups = &a.src[i];
        Cin += t.C;
        if (i == 0) a.c1 = Cin;
        if (i <= 1) a.c2 = Cin;
    }
    a.Cin = Cin;
    a.Hout = a.Hin; a.Wout = a.Win;
    const int H = a.Hout, W = a.Wout;
    std::vector<float> wk((size_t)Cin * 9 * a.CoutPad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < 9; ++k) wk[((size_t)ci * 9 + k) * a.CoutPad + co] = in[0][((size_t)co * Cin + ci) * 9 + k];
    DevBuf dwk(wk.data(), wk.size());
    a.w = dwk.p;
    a.epi = upload(in[1], (size_t)Cout * 2); a.epi_slope = fp[0];
    LocalConv wf;
    debug_weight_forms(dwk.p, Cin, 3, 1, 1, 1, a.CoutPad, a.Win, true, a, wf);
    VR_CHECK(a.x3w && conv_plan(a, ConvShape{3, 1, 1, 1}).k == CK_X3, -2, who + "conv_x3h does not take this launch");
    // the second stage: K-major weights [Cout][CoutPad2] (kind 1) or [Cout] (kind 2)
    const int CoutPad2 = (Cout2 + 31) / 32 * 32;
    std::vector<float> w2((size_t)Cout * (kind == 1 ? CoutPad2 : 1), 0.f);
    for (int j = 0; j < Cout2; ++j)
        for (int c = 0; c < Cout; ++c) w2[kind == 1 ? (size_t)c * CoutPad2 + j : (size_t)c] = in[2][(size_t)j * Cout + c];
    DevBuf dw2(w2.data(), w2.size());
    const float* epi2 = upload(in[3], (size_t)Cout2 * 2);
    const size_t yfloats = (size_t)dims[7];
    const long long yoff = kind == 1 ? dims[8] : 0, ysN = kind == 1 ? dims[9] : (long long)H * W, ysC = kind == 1 ? dims[10] : 0,
                    ysH = kind == 1 ? dims[11] : W;
    VR_CHECK(view_fits(yoff, ysN, kind == 1 ? ysC : 1, ysH, N, kind == 1 ? Cout2 : 1, H, W, yfloats), -2, who + "the view of y leaves its buffer");
    GuardedBuf y(in[4], yfloats);
    DevBuf prod((size_t)N * Cout * H * W);
    a.dst[0] = ConvDst{prod.p, (long long)Cout * H * W, (long long)H * W, W, 0, 0};
    conv_fill_tiling(a, tile);
    if (fuse_tail) {
        a.tail = kind; a.t_Cout = Cout2; a.t_CoutPad = kind == 1 ? CoutPad2 : 1; a.t_w = dw2.p; a.t_epi = epi2; a.t_slope = fp[1];
        a.t_p = y.p() + yoff; a.t_sN = ysN; a.t_sC = ysC; a.t_sH = ysH;
        VR_CHECK(x3h_tail_ok(a, tile), -2, who + "conv_x3h has no kernel for this launch with a second stage (x3h_tail_ok)");
        x3h_launch_conv(a, tile, stream);
    } else {
        x3h_launch_conv(a, tile, stream);
        const Tensor pt = dense(prod.p, N, Cout, H, W);
        if (kind == 1) {
            ConvArgs b{};
            b.nsrc = 1; b.N = N; b.Cin = Cout; b.c1 = b.c2 = Cout; b.Cout = Cout2; b.CoutPad = CoutPad2;
            b.d1 = b.d2 = 1 << 30;
            b.bf16 = 3;
            b.src[0] = make_src(pt, false, 0);
            b.Hin = b.Hout = H; b.Win = b.Wout = W;
            b.w = dw2.p;
            b.epi = epi2; b.epi_slope = fp[1];
            b.dst[0] = ConvDst{y.p() + yoff, ysN, ysC, ysH, 0, 0};
            launch_conv(b, ConvShape{1, 1, 1, 1}, stream);
        } else {
            launch_squeeze_conv(pt, dw2.p, y.p(), nullptr, false, stream, epi2);
        }
    }
    VR_HIP(hipStreamSynchronize(stream));
    VR_CHECK(y.intact(), -3, who + "a launch stored outside y's buffer");
    y.download(out[0]);
    prod.download(out[1]);
}

void Model::debug_wgrad_launch(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                               int nout) {
    const std::string who = "vr_debug_kernel(wgrad_launch): ";
    VR_CHECK(ndims >= 13 && nfp >= 3 && nin >= 2 && nout >= 2, -2, who + "too few arguments");
    const int nsrc = (int)dims[0], N = (int)dims[1], Cout = (int)dims[2], KS = (int)dims[3], stride = (int)dims[4];
    const int dh = (int)dims[5], dw = (int)dims[6], flags = (int)dims[7];
    const bool batch_as_h = flags & 1, accumulate = flags & 2, defer = flags & 4, twice = flags & 8, accumulate2 = flags & 16;
    VR_CHECK(nsrc >= 1 && nsrc <= 3 && N >= 1 && Cout >= 1 && (KS == 1 || KS == 3) && (stride == 1 || stride == 2) && dh >= 1 && dw >= 1, -2,
             who + "1..3 sources, a 1x1 or 3x3 kernel, stride 1 or 2");
    VR_CHECK(ndims >= 13 + 10 * nsrc && nin >= 2 + 4 * nsrc, -2, who + "too few arguments");
    VR_CHECK(in[0] && in[1] && out[0] && out[1], -2, who + "missing dz, gradient or an output");
    WgradArgs w{};
    ConvArgs& a = w.in;
    a.nsrc = nsrc; a.Cout = Cout; a.CoutPad = (Cout + 31) / 32 * 32;
    a.d1 = a.d2 = 1 << 30;
    a.pad_h = KS == 1 ? 0 : dh; a.pad_w = KS == 1 ? 0 : dw;
    std::vector<std::unique_ptr<DevBuf>> keep;
    auto upload = [&](const float* host, size_t n) { keep.emplace_back(new DevBuf(host, n)); return keep.back()->p; };
    int Cin = 0, Hin = 0, Win = 0;
    const ConvSrc* ups = nullptr;
    for (int i = 0; i < nsrc; ++i) {
        const int64_t* d = dims + 13 + 10 * i;
        const float* const* si = in + 2 + 4 * i;
        Tensor t;
        t.N = N; t.C = (int)d[0]; t.H = (int)d[1]; t.W = (int)d[2];
        const bool up = d[3] != 0;
        t.hsplit = (int)d[4];
        const size_t floats = (size_t)d[5];
        t.sN = d[7]; t.sC = d[8]; t.sH = d[9];
        VR_CHECK(si[0] && view_fits(d[6], t.sN, t.sC, t.sH, N, t.C, t.H, t.W, floats), -2, who + "a source view leaves its buffer");
        t.p = upload(si[0], floats) + d[6];
        t.slope = fp[i];
        if (si[1]) t.aff0 = upload(si[1], (size_t)t.C * 2);
        if (si[2]) t.aff1 = upload(si[2], (size_t)t.C * 2);
        if (si[3]) t.post = upload(si[3], (size_t)N * t.C);
        a.src[i] = make_src(t, up, 0);
        const int vh = up ? 2 * t.H : t.H, vw = up ? 2 * t.W : t.W;
        if (i == 0) { Hin = vh; Win = vw; }
        VR_CHECK(vh == Hin && vw == Win, -2, who + "the sources must share the input size");
        if (up && ups) VR_CHECK(ups->H == t.H && ups->W == t.W && ups->sH == t.sH, -2, who + "upsampled sources must share H, W and row stride");
        if (up) ups = &a.src[i];
        Cin += t.C;
        if (i == 0) a.c1 = Cin;
        if (i <= 1) a.c2 = Cin;
    }
    a.Cin = Cin;
    if (nsrc < 2) a.c1 = Cin;                                 // (Model::build_fwd_args: a missing source is an empty range at the end)
    if (nsrc < 3) a.c2 = Cin;
    // the dz view, before the batch-as-rows rewrite: [N][Cout][Hout][Wout]
    const int Hout0 = (Hin + 2 * a.pad_h - dh * (KS - 1) - 1) / stride + 1, Wout = (Win + 2 * a.pad_w - dw * (KS - 1) - 1) / stride + 1;
    VR_CHECK(Hout0 >= 1 && Wout >= 1, -2, who + "empty output");
    const size_t zfloats = (size_t)dims[8];
    VR_CHECK(view_fits(dims[9], dims[10], dims[11], dims[12], N, Cout, Hout0, Wout, zfloats), -2, who + "the dz view leaves its buffer");
    DevBuf dz(in[0], zfloats);
    w.dz = dz.p + dims[9];
    int Nk = N;
    if (batch_as_h) {                                         // Model::build_fwd_args' and Model::bwd_conv's rewrites
        VR_CHECK(KS == 1 && Hin == 1, -2, who + "batch-as-rows view needs a 1x1 conv on H=1 input");
        for (int i = 0; i < nsrc; ++i) {
            VR_CHECK(!a.src[i].post && !a.src[i].up, -2, who + "batch-as-rows: unsupported source flags");
            a.src[i].sH = a.src[i].sN; a.src[i].sN = 0; a.src[i].H = N;
        }
        Hin = N; Nk = 1;
        w.zN = 0; w.zC = dims[11]; w.zH = dims[10];
    } else {
        w.zN = dims[10]; w.zC = dims[11]; w.zH = dims[12];
    }
    a.N = Nk; a.Hin = Hin; a.Win = Win;
    a.Hout = (Hin + 2 * a.pad_h - dh * (KS - 1) - 1) / stride + 1; a.Wout = Wout;
    w.Cout = Cout; w.CoutPad = a.CoutPad;
    w.allow_wino = train_wino ? 1 : 0;
    w.bf16 = mfma_mode;
    const ConvShape shp{KS, stride, dh, dw};
    // the plan launch_wgrad launches (it calls the same wgrad_choose on the same arguments), for P and part_stride
    WgradArgs pl = w;
    {
        int CB = 0, MT = 0;
        wgrad_choose(pl, shp, &CB, &MT);
    }
    const size_t gfloats = (size_t)Cin * KS * KS * a.CoutPad, sfloats = wgrad_scratch_floats(w, shp);
    VR_CHECK((size_t)pl.P * (size_t)pl.part_stride <= sfloats, -4, who + "the plan's slabs exceed wgrad_scratch_floats");
    GuardedBuf grad(in[1], gfloats);
    const std::vector<float> nans(sfloats, std::nanf(""));
    GuardedBuf scratch(nans.data(), sfloats), scratch2(twice ? nans.data() : nullptr, twice ? sfloats : 0);
    w.part = scratch.p();
    long long ndesc = 0;
    {
        struct Unsink {                                   // (also when a launch throws: no descriptor of freed buffers stays behind)
            std::vector<WgReduceDesc>& v;
            ~Unsink() { wgrad_defer_to(nullptr); v.clear(); }
        } unsink{wred_host};
        wred_host.clear();
        if (defer) wgrad_defer_to(&wred_host);
        launch_wgrad(w, shp, grad.p(), accumulate ? 1 : 0, stream);
        if (twice) {
            w.part = scratch2.p();
            launch_wgrad(w, shp, grad.p(), accumulate2 ? 1 : 0, stream);
        }
        wgrad_defer_to(nullptr);
        ndesc = (long long)wred_host.size();
        for (const WgReduceDesc& d : wred_host)
            VR_CHECK(d.P == pl.P && d.stride == pl.part_stride && d.n == pl.part_stride, -4, who + "the deferred descriptor is not the plan's");
        flush_wgrad_sums();
    }
    VR_HIP(hipStreamSynchronize(stream));
    VR_CHECK(grad.intact() && scratch.intact() && scratch2.intact(), -3, who + "the launch stored outside the gradient or the scratch slab");
    grad.download(out[0]);
    const int64_t info[4] = {pl.P, pl.part_stride, (int64_t)sfloats, ndesc};
    std::memcpy(out[1], info, sizeof info);
}

void Model::debug_dgrad_launch(const int64_t* dims, int ndims, const float* const* in, int nin, float* const* out, int nout) {
    const std::string who = "vr_debug_kernel(dgrad_launch): ";
    VR_CHECK(ndims >= 13 && nin >= 2, -2, who + "too few arguments");
    const int nsrc = (int)dims[0], N = (int)dims[1], Cout = (int)dims[2], KS = (int)dims[3], stride = (int)dims[4];
    const int dh = (int)dims[5], dw = (int)dims[6], flags = (int)dims[7];
    const bool batch_as_h = flags & 1;
    VR_CHECK(nsrc >= 1 && nsrc <= 3 && N >= 1 && Cout >= 1 && (KS == 1 || KS == 3) && (stride == 1 || stride == 2) && dh >= 1 && dw >= 1, -2,
             who + "1..3 sources, a 1x1 or 3x3 kernel, stride 1 or 2");
    VR_CHECK(stride == 1 || (KS == 3 && dh == 1 && dw == 1), -2, who + "stride 2 needs a 3x3 kernel without dilation");
    VR_CHECK(ndims >= 13 + 11 * nsrc && nin >= 2 + nsrc && nout >= nsrc + 1, -2, who + "too few arguments");
    VR_CHECK(in[0] && in[1] && out[nsrc], -2, who + "missing weights, dz or the info output");
    LocalConv lc;
    Conv& L = lc.L;
    Param& P = lc.P;
    L.name = "debug"; L.KS = KS; L.stride = stride; L.dh = dh; L.dw = dw;
    L.pad_h = KS == 1 ? 0 : dh; L.pad_w = KS == 1 ? 0 : dw; L.bn = nullptr; L.slope = 1.f;
    TapeRec r;
    r.kind = TK_CONV; r.L = &L; r.N = N; r.batch_as_h = batch_as_h;
    // sources: only their shapes and gradient views matter to a data gradient
    std::vector<std::unique_ptr<GuardedBuf>> grads(nsrc);
    struct Unfresh {                                      // (also when a launch throws: no entry of a freed buffer stays behind)
        std::map<const float*, bool>& fresh;
        std::vector<const float*> keys;
        ~Unfresh() { for (const float* k : keys) fresh.erase(k); }
    } unfresh{g_fresh, {}};
    int Cin = 0, Hin = 0, Win = 0;
    for (int i = 0; i < nsrc; ++i) {
        const int64_t* d = dims + 13 + 11 * i;
        Tensor t;
        t.N = N; t.C = (int)d[0]; t.H = (int)d[1]; t.W = (int)d[2];
        const bool up = d[3] != 0;
        const int bcastH = (int)d[4], mode = (int)d[5];
        const size_t floats = (size_t)d[6];
        t.sN = d[8]; t.sC = d[9]; t.sH = d[10];
        VR_CHECK(mode >= 0 && mode <= 2 && bcastH >= 0 && !(up && bcastH), -2, who + "mode is 0, 1 or 2; a source is upsampled or broadcast, not both");
        VR_CHECK(in[2 + i] && out[i], -2, who + "every source needs its gradient buffer, in and out");
        VR_CHECK(view_fits(d[7], t.sN, t.sC, t.sH, N, t.C, t.H, t.W, floats), -2, who + "a gradient view leaves its buffer");
        if (bcastH) VR_CHECK(t.H == 1 && t.sC == t.W && t.sN == (long long)t.C * t.W, -2, who + "a broadcast source has H = 1 and a dense gradient");
        grads[i].reset(new GuardedBuf(in[2 + i], floats));
        if (mode) t.g = grads[i]->p() + d[7];
        if (mode == 1) { g_fresh[t.g] = true; unfresh.keys.push_back(t.g); }
        SrcSpec sp{t};
        sp.up = up; sp.bcastH = bcastH;
        r.srcs.push_back(sp);
        const int vh = up ? 2 * t.H : (bcastH ? bcastH : t.H), vw = up ? 2 * t.W : t.W;
        if (i == 0) { Hin = vh; Win = vw; }
        VR_CHECK(vh == Hin && vw == Win, -2, who + "the sources must share the input size");
        Cin += t.C;
    }
    L.Cin = Cin; L.Cout = Cout; L.CoutPad = (Cout + 31) / 32 * 32;
    const int KK = KS * KS;
    P.kind = PK_CONV; P.Cin = Cin; P.Cout = Cout; P.KK = KK; P.CoutPad = L.CoutPad;
    std::vector<float> wk((size_t)Cin * KK * L.CoutPad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < KK; ++k) wk[((size_t)ci * KK + k) * L.CoutPad + co] = in[0][((size_t)co * Cin + ci) * KK + k];
    DevBuf dwk(wk.data(), wk.size());
    P.dev = dwk.p;
    // dz: the view [N][Cout][Hout][Wout] of its buffer
    const int Hout = (Hin + 2 * L.pad_h - dh * (KS - 1) - 1) / stride + 1, Wout = (Win + 2 * L.pad_w - dw * (KS - 1) - 1) / stride + 1;
    VR_CHECK(Hout >= 1 && Wout >= 1, -2, who + "empty output");
    const size_t zfloats = (size_t)dims[8];
    VR_CHECK(view_fits(dims[9], dims[10], dims[11], dims[12], N, Cout, Hout, Wout, zfloats), -2, who + "the dz view leaves its buffer");
    DevBuf dz(in[1], zfloats);
    r.out.p = nullptr; r.out.g = dz.p + dims[9]; r.out.N = N; r.out.C = Cout; r.out.H = Hout; r.out.W = Wout;
    r.out.sN = dims[10]; r.out.sC = dims[11]; r.out.sH = dims[12]; r.out.slope = 1.f;
    ConvArgs f;
    build_fwd_args(L, r.srcs, N, batch_as_h, f);          // (refuses a batch-as-rows record that is no 1x1 conv on H = 1)
    debug_dgrad_weight_forms(lc);
    // the workspace: sized by a dry pass, then a guarded slab of exactly that size in place of the handle's arena
    struct WsRestore {
        Model* m; Arena saved;
        ~WsRestore() { m->ws = saved; m->dry = false; }
    } ws_restore{this, ws};
    ws.dry = true; ws.base = nullptr; ws.off = 0; ws.peak = 0; dry = true;
    bwd_conv_dgrad(r, f);
    dry = false;
    const size_t wfloats = (ws.peak + 3) / 4;
    const std::vector<float> nans(wfloats, std::nanf(""));
    GuardedBuf wsbuf(nans.data(), wfloats);
    ws = Arena{};
    ws.base = reinterpret_cast<char*>(wsbuf.p()); ws.cap = wfloats * 4;
    int path = DG_NONE;
    try {
        path = bwd_conv_dgrad(r, f);
    } catch (...) {                                       // a refusal: the caller still sees what the buffers hold (nothing may have been written)
        (void)hipStreamSynchronize(stream);
        for (int i = 0; i < nsrc; ++i) grads[i]->download(out[i]);
        throw;
    }
    VR_HIP(hipStreamSynchronize(stream));
    bool intact = wsbuf.intact();
    for (int i = 0; i < nsrc; ++i) intact = intact && grads[i]->intact();
    VR_CHECK(intact, -3, who + "the launch stored outside a gradient buffer or the workspace");
    for (int i = 0; i < nsrc; ++i) grads[i]->download(out[i]);
    const int64_t info[4] = {path, (int64_t)wfloats, 0, 0};
    std::memcpy(out[nsrc], info, sizeof info);
}

void Model::debug_wgrad_reduce(const int64_t* dims, int ndims, const float* const* in, int nin, float* const* out, int nout) {
    const std::string who = "vr_debug_kernel(wgrad_reduce): ";
    VR_CHECK(ndims >= 1, -2, who + "too few arguments");
    const int nd = (int)dims[0];
    VR_CHECK(nd >= 1 && nd <= 128 && ndims >= 1 + 6 * nd && nin >= 2 * nd && nout >= 2 * nd + 1, -2, who + "1..128 descriptors, six dims each");
    std::vector<std::unique_ptr<DevBuf>> slabs;
    std::vector<std::unique_ptr<GuardedBuf>> o_imm, o_bat;
    std::vector<WgReduceDesc> descs;
    for (int j = 0; j < nd; ++j) {
        const int64_t* d = dims + 1 + 6 * j;
        const long long P = d[0], n = d[1], stride = d[2], floats = d[4], off = d[5];
        VR_CHECK(P >= 1 && n >= 1 && stride >= n && off >= 0 && off + n <= floats, -2, who + "need P, n >= 1, stride >= n and the output inside its buffer");
        VR_CHECK(in[2 * j] && in[2 * j + 1] && out[2 * j] && out[2 * j + 1] && out[2 * nd], -2, who + "missing buffer");
        slabs.emplace_back(new DevBuf(in[2 * j], (size_t)(P * stride)));
        o_imm.emplace_back(new GuardedBuf(in[2 * j + 1], (size_t)floats));
        o_bat.emplace_back(new GuardedBuf(in[2 * j + 1], (size_t)floats));
        descs.push_back(WgReduceDesc{slabs.back()->p, stride, o_bat.back()->p() + off, n, (int)P, d[3] != 0 ? 1 : 0, 0});
    }
    for (int j = 0; j < nd; ++j) {
        const WgReduceDesc& d = descs[j];
        launch_wgrad_reduce(d.part, d.stride, d.P, o_imm[j]->p() + dims[1 + 6 * j + 5], d.n, d.accumulate, stream);
    }
    const int vec = wgrad_reduce_vec(descs.data(), nd);
    wred_host = descs;
    flush_wgrad_sums();
    VR_HIP(hipStreamSynchronize(stream));
    for (int j = 0; j < nd; ++j) {
        VR_CHECK(o_imm[j]->intact() && o_bat[j]->intact(), -3, who + "a slab sum stored outside its output buffer");
        o_imm[j]->download(out[2 * j]);
        o_bat[j]->download(out[2 * j + 1]);
    }
    out[2 * nd][0] = (float)vec;
}

void Model::debug_kernel(const std::string& name, const int64_t* dims, int ndims, const float* fp, int nfp,
                         const float* const* in, int nin, float* const* out, int nout) {
    DeviceGuard dev_guard(device);
    auto need = [&](int nd, int nf, int ni, int no) {
        VR_CHECK(ndims >= nd && nfp >= nf && nin >= ni && nout >= no, -2, "vr_debug_kernel(" + name + "): too few arguments");
    };
    hipStream_t st = stream;
    if (name == "x3h_trace") {
        // conv_x3h.hip phase stamps (VR_CONV_DBG bit 64).  dims[0]: 0 = clear, 1 = read into out[0] (768 floats: cycles relative to the
        // earliest stamp, -1 where nothing was stamped); layout [workgroup 4][wave 4][chunk 6][point 8]
        need(1, 0, 0, dims[0] ? 1 : 0);
        VR_HIP(hipDeviceSynchronize());
        if (!dims[0]) { x3h_trace_clear(); return; }
        long long raw[768];
        x3h_trace_read(raw, 768);
        long long lo = 0;
        for (long long v : raw) if (v && (!lo || v < lo)) lo = v;
        for (int i = 0; i < 768; ++i) out[0][i] = raw[i] ? (float)(raw[i] - lo) : -1.f;
        return;
    }
    if (name == "conv_launch") { debug_conv_launch(dims, ndims, fp, nfp, in, nin, out, nout); return; }
    if (name == "conv_tail") { debug_conv_tail(dims, ndims, fp, nfp, in, nin, out, nout); return; }
    if (name == "wgrad_launch") { debug_wgrad_launch(dims, ndims, fp, nfp, in, nin, out, nout); return; }
    if (name == "wgrad_reduce") { debug_wgrad_reduce(dims, ndims, in, nin, out, nout); return; }
    if (name == "dgrad_launch") { debug_dgrad_launch(dims, ndims, in, nin, out, nout); return; }
    if (name == "tensor_pass") { debug_tensor_pass(dims, ndims, fp, nfp, in, nin, out, nout); return; }
    if (name == "weight_forms") { debug_weight_form_launch(dims, ndims, in, nin, out, nout); return; }
    if (name == "layer_forms") { debug_layer_forms(dims, ndims, out, nout); return; }
    if (name == "bn_backward") {
        need(4, 3, 7, 6);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3];
        // optional: z and G as a view of a wider buffer, and the broadcast affine table of BatchNorm(1)
        const bool view = ndims >= 10;
        const long long off = view ? dims[5] : 0, sH = view ? dims[8] : W, sC = view ? dims[7] : (long long)H * W, sN = view ? dims[6] : sC * C;
        const size_t n = view ? (size_t)dims[4] : (size_t)N * C * H * W;
        const int aff_bcast = view && dims[9] != 0 ? 1 : 0;
        VR_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1, -2, "bn_backward: empty tensor");
        VR_CHECK(view_fits(off, sN, sC, sH, N, C, H, W, n), -2, "bn_backward: the view leaves its buffer");
        VR_CHECK(!aff_bcast || C == 1, -2, "bn_backward: a broadcast affine table belongs to a single-channel BatchNorm");
        DevBuf z(in[0], n), gamma(in[2], C), beta(in[3], C), rm(in[5], C), rv(in[6], C);
        GuardedBuf g(in[1], n);
        DevBuf post(in[4], in[4] ? (size_t)N * C : 0);
        // forward statistics: one partial row of (sum, sumsq) per channel, then the library's own finalize
        std::vector<float> part((size_t)C * 2);
        for (int c = 0; c < C; ++c) {
            double s1 = 0, s2 = 0;
            for (int b = 0; b < N; ++b)
                for (int h = 0; h < H; ++h) {
                    const float* q = in[0] + off + b * sN + c * sC + h * sH;
                    for (int i = 0; i < W; ++i) { s1 += q[i]; s2 += (double)q[i] * q[i]; }
                }
            part[2 * c] = (float)s1; part[2 * c + 1] = (float)s2;
        }
        const int bcast_rows = aff_bcast ? 8 : 0;             // (the squeeze BatchNorm's table is one row per frequency bin, all equal)
        DevBuf dpart(part.data(), part.size()), aff((size_t)(aff_bcast ? bcast_rows : C) * 2), smean(C), sinv(C), dgamma(C), dbeta(C);
        BNFinalizeArgs f{};
        f.part = dpart.p; f.nparts = 1; f.pstride = C * 2; f.count = (double)N * H * W;
        f.w = gamma.p; f.b = beta.p; f.rm = rm.p; f.rv = rv.p; f.affine = aff.p; f.save_mean = smean.p; f.save_invstd = sinv.p;
        f.C = C; f.eps = fp[1]; f.momentum = fp[2]; f.broadcast = bcast_rows;
        launch_bn_finalize(f, st);
        BnBwdArgs a{};
        a.g = g.p() + off; a.z = z.p + off; a.N = N; a.C = C; a.H = H; a.W = W; a.sH = sH; a.sC = sC; a.sN = sN;
        a.aff = aff.p; a.aff_bcast = aff_bcast; a.slope = fp[0]; a.post = in[4] ? post.p : nullptr;
        a.gamma = gamma.p; a.save_mean = smean.p; a.save_invstd = sinv.p; a.dgamma = dgamma.p; a.dbeta = dbeta.p; a.acc_grads = 1;
        DevBuf coef((size_t)C * 3), bpart((size_t)bn_bwd_chunks(a) * C * 2);
        a.coef = coef.p; a.part = bpart.p;
        launch_bn_bwd(a, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(g.intact(), -3, "bn_backward: a store outside the gradient's buffer");
        g.download(out[0]); dgamma.download(out[1]); dbeta.download(out[2]); rm.download(out[4]); rv.download(out[5]);
        if (out[3]) VR_HIP(hipMemcpy(out[3], aff.p, (size_t)C * 2 * sizeof(float), hipMemcpyDeviceToHost));
    } else if (name == "lstm") {
        const int flags = ndims >= 4 ? (int)dims[3] : 0;
        const bool infer = flags & 1, bwd_only = flags & 2;
        need(3, 0, infer ? 3 : 4, infer ? 1 : 4);
        const int N = (int)dims[0], T = (int)dims[1], H = (int)dims[2], G = 4 * H;
        VR_CHECK(N > 0 && T > 0 && H > 0, -2, "lstm: N, T, H must be positive");
        DevBuf gx(in[0], (size_t)N * 2 * G * T), wf(in[1], (size_t)G * H), wr(in[2], (size_t)G * H), h((size_t)N * 2 * H * T);
        if (infer) {
            launch_bilstm(gx.p, wf.p, wr.p, h.p, N, T, H, st);
            VR_HIP(hipStreamSynchronize(st));
            h.download(out[0]);
            return;
        }
        DevBuf dh(in[3], (size_t)N * 2 * H * T), save((size_t)N * 2 * T * 5 * H), dgx((size_t)N * 2 * G * T);
        // launch_lstm_whh_grad below accumulates: onto the caller's initial gradients, or onto zeros
        const float* f0 = nin >= 5 ? in[4] : nullptr;
        const float* r0 = nin >= 6 ? in[5] : nullptr;
        std::vector<float> zeros(f0 && r0 ? 0 : (size_t)G * H, 0.f);
        DevBuf dwf(f0 ? f0 : zeros.data(), (size_t)G * H), dwr(r0 ? r0 : zeros.data(), (size_t)G * H);
        if (!bwd_only) launch_bilstm_train(gx.p, wf.p, wr.p, h.p, save.p, N, T, H, st);
        launch_bilstm_bwd(dh.p, save.p, wf.p, wr.p, dgx.p, N, T, H, st);
        DevBuf wpart(lstm_whh_grad_scratch_floats(N, H));
        launch_lstm_whh_grad(dgx.p, h.p, dwf.p, dwr.p, N, T, H, 1, wpart.p, st);
        VR_HIP(hipStreamSynchronize(st));
        h.download(out[0]); dgx.download(out[1]); dwf.download(out[2]); dwr.download(out[3]);
    } else if (name == "upsample") {
        need(4, 0, 2, 2);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3];
        const size_t n = (size_t)N * C * H * W;
        // optional: the low-resolution gradient as a view of its own buffer (prior contents in[2]), stored into or accumulated into
        const bool view = ndims >= 10;
        const long long off = view ? dims[5] : 0, gN = view ? dims[6] : (long long)C * H * W, gC = view ? dims[7] : (long long)H * W, gH = view ? dims[8] : W;
        const size_t gfloats = view ? (size_t)dims[4] : n;
        VR_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1, -2, "upsample: empty tensor");
        VR_CHECK(!view || (nin >= 3 && in[2]), -2, "upsample: a strided gradient needs its backing buffer");
        VR_CHECK(view_fits(off, gN, gC, gH, N, C, H, W, gfloats), -2, "upsample: the gradient view leaves its buffer");
        const std::vector<float> zeros(view ? 0 : n, 0.f);
        DevBuf x(in[0], n), dhi(in[1], 4 * n), up(4 * n);
        GuardedBuf glo(view ? in[2] : zeros.data(), gfloats);
        launch_upsample2x(dense(x.p, N, C, H, W), up.p, st);
        launch_upsample_bwd(dhi.p, N, C, H, W, glo.p() + off, gN, gC, gH, view ? (dims[9] != 0 ? 1 : 0) : 1, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(glo.intact(), -3, "upsample: a store outside the gradient's buffer");
        up.download(out[0]); glo.download(out[1]);
    } else if (name == "pool") {
        need(4, 0, 3, 3);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3];
        const size_t n = (size_t)N * C * H * W, m = (size_t)N * C * W;
        const bool view = ndims >= 10;
        const long long off = view ? dims[5] : 0, gN = view ? dims[6] : (long long)C * H * W, gC = view ? dims[7] : (long long)H * W, gH = view ? dims[8] : W;
        const size_t gfloats = view ? (size_t)dims[4] : n;
        VR_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1, -2, "pool: empty tensor");
        VR_CHECK(!view || (nin >= 4 && in[3]), -2, "pool: a strided gradient needs its backing buffer");
        VR_CHECK(view_fits(off, gN, gC, gH, N, C, H, W, gfloats), -2, "pool: the gradient view leaves its buffer");
        const std::vector<float> zeros(view ? 0 : n, 0.f);
        DevBuf x(in[0], n), gp(in[1], m), d(in[2], n), pooled(m), sumh(m);
        GuardedBuf g(view ? in[3] : zeros.data(), gfloats);
        launch_avgpool_h(dense(x.p, N, C, H, W), pooled.p, st);
        launch_avgpool_bwd(gp.p, g.p() + off, N, C, H, W, gN, gC, gH, view ? (dims[9] != 0 ? 1 : 0) : 1, st);
        launch_sum_h(d.p, N, C, H, W, sumh.p, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(g.intact(), -3, "pool: a store outside the gradient's buffer");
        pooled.download(out[0]); g.download(out[1]); sumh.download(out[2]);
    } else if (name == "thin") {
        need(5, 1, 4, 3);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3], CO = (int)dims[4];
        VR_CHECK(CO == 1 || CO == 2, -2, "thin: CO must be 1 or 2");
        const size_t n = (size_t)N * C * H * W, nz = (size_t)N * CO * H * W;
        DevBuf x(in[0], n), aff(in[1], in[1] ? (size_t)C * 2 : 0), w(in[2], (size_t)CO * C), dz(in[3], nz), g(n), dw((size_t)CO * C);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0];
        if (in[1]) t.aff0 = aff.p;
        DevBuf part((size_t)thin_wgrad_blocks(t) * CO * C);
        launch_thin_dgrad(t, CO, w.p, dz.p, g.p, 0, st);          // store, then accumulate once more: the caller expects 2 x the gradient
        launch_thin_dgrad(t, CO, w.p, dz.p, g.p, 1, st);
        launch_thin_wgrad(t, CO, dz.p, part.p, dw.p, 0, st);
        DevBuf zf((size_t)N * H * W);
        if (CO == 1) launch_squeeze_conv(t, w.p, zf.p, nullptr, false, st);
        VR_HIP(hipStreamSynchronize(st));
        g.download(out[0]); dw.download(out[1]);
        if (CO == 1) zf.download(out[2]);
    } else if (name == "head_loss") {
        need(5, 2, 5, 3);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3], bins = (int)dims[4];
        const size_t n = (size_t)N * C * H * W, nx = (size_t)N * 2 * bins * W;
        DevBuf x(in[0], n), aff(in[1], in[1] ? (size_t)C * 2 : 0), w(in[2], (size_t)2 * C), X(in[3], nx), Y(in[4], nx);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0];
        if (in[1]) t.aff0 = aff.p;
        DevBuf dlogit((size_t)N * 2 * H * W), mask(nx), lpart((size_t)head_loss_blocks(t)), loss(4);
        HeadScratch hs{};
        hs.dlogit = dlogit.p; hs.lpart = lpart.p;
        run_train_head(plan, t, TrainHead{0, false, w.p, X.p, Y.p, bins, mask.p, loss.p, (float)(1.0 / (double)nx), fp[1], 0.f, nullptr, 0, nullptr, 0},
                       hs, nullptr, st);
        VR_HIP(hipStreamSynchronize(st));
        dlogit.download(out[0]); mask.download(out[1]);
        VR_HIP(hipMemcpy(out[2], loss.p, sizeof(float), hipMemcpyDeviceToHost));
    } else if (name == "head_loss_complex") {
        need(5, 2, 5, 5);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3], bins = (int)dims[4];
        VR_CHECK(N > 0 && C > 0 && H > 0 && W > 0 && bins >= H && W % 4 == 0, -2, "head_loss_complex: need positive sizes, bins >= H, W % 4 == 0");
        const size_t n = (size_t)N * C * H * W, nx = (size_t)N * 2 * bins * W;       // (nx complex elements)
        DevBuf x(in[0], n), aff(in[1], in[1] ? (size_t)C * 2 : 0), w(in[2], (size_t)4 * C), X(in[3], 2 * nx), Y(in[4], 2 * nx);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0];
        if (in[1]) t.aff0 = aff.p;
        DevBuf dlogit((size_t)N * 4 * H * W), mask(2 * nx), lpart((size_t)head_loss_blocks(t)), loss(4), g(n), dw((size_t)4 * C);
        DevBuf part((size_t)thin_wgrad_blocks(t) * 4 * C);
        HeadScratch hs{};
        hs.dlogit = dlogit.p; hs.lpart = lpart.p; hs.wpart = part.p;
        run_train_head(plan, t, TrainHead{0, true, w.p, X.p, Y.p, bins, mask.p, loss.p, (float)(1.0 / (double)nx), fp[1], 0.f, g.p, 0, dw.p, 0},
                       hs, nullptr, st);
        VR_HIP(hipStreamSynchronize(st));
        dlogit.download(out[0]); mask.download(out[1]);
        VR_HIP(hipMemcpy(out[2], loss.p, sizeof(float), hipMemcpyDeviceToHost));
        g.download(out[3]); dw.download(out[4]);
    } else if (name == "head") {
        need(11, 1, 4, 1);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3], w_lo = (int)dims[4], w_hi = (int)dims[5];
        const int pad_rows = (int)dims[6], hsplit = (int)dims[8], pitch_extra = (int)dims[10];
        const bool cplx = dims[7] != 0, use_items = dims[9] != 0;
        VR_CHECK(N > 0 && C > 0 && H > 0 && W > 0 && pad_rows >= 0 && pitch_extra >= 0 && w_lo >= 0 && w_hi <= W && w_lo <= w_hi, -2,
                 "head: need positive sizes and 0 <= w_lo <= w_hi <= W");
        VR_CHECK(!use_items || nout >= N, -2, "head: use_items needs one output per item");
        const int CO = cplx ? 4 : 2, E = cplx ? 2 : 1, Wm = w_hi - w_lo, rows = H + pad_rows;
        const size_t n = (size_t)N * C * H * W;
        DevBuf x(in[0], n), aff0(in[1], in[1] ? (size_t)C * 2 : 0), aff1(in[2], in[2] ? (size_t)C * 2 : 0), w(in[3], (size_t)CO * C);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0]; t.hsplit = hsplit;
        if (in[1]) t.aff0 = aff0.p;
        if (in[2]) t.aff1 = aff1.p;
        // one destination per item (use_items; item n has its own pitch) or one dense destination, all NaN before the launch
        const int nbuf = use_items ? N : 1;
        std::vector<std::unique_ptr<DevBuf>> dst;
        std::vector<float*> items_h;
        std::vector<int> pitch_h;
        for (int b = 0; b < nbuf; ++b) {
            const int pitch = Wm + pitch_extra + (use_items ? b : 0);
            const size_t words = (size_t)(use_items ? 1 : N) * 2 * rows * pitch * E;
            const std::vector<float> fill(words, std::nanf(""));
            dst.emplace_back(new DevBuf(fill.data(), words));
            items_h.push_back(dst.back()->p);
            pitch_h.push_back(pitch);
        }
        DevBuf items_d((size_t)N * 2), pitch_d((size_t)N);         // device tables: N pointers, N ints
        HeadDst d{};
        d.w_lo = w_lo; d.w_hi = w_hi; d.pad_rows = pad_rows;
        if (use_items) {
            VR_HIP(hipMemcpy(items_d.p, items_h.data(), (size_t)N * sizeof(float*), hipMemcpyHostToDevice));
            VR_HIP(hipMemcpy(pitch_d.p, pitch_h.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
            d.items = reinterpret_cast<float* const*>(items_d.p);
            d.item_pitch = reinterpret_cast<const int*>(pitch_d.p);
        } else {
            d.p = dst[0]->p; d.dH = pitch_h[0]; d.dC = (long long)rows * d.dH; d.dN = 2 * d.dC;
        }
        if (cplx) launch_head_complex(t, w.p, d, st);
        else launch_head_sigmoid(t, w.p, d, st);
        VR_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < nbuf; ++b) dst[b]->download(out[b]);
    } else if (name == "squeeze") {
        need(5, 1, 4, 1);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3];
        const bool use_part = dims[4] != 0;
        VR_CHECK(N > 0 && C > 0 && H > 0 && W > 0, -2, "squeeze: sizes must be positive");
        VR_CHECK(!use_part || (nout >= 2 && out[1]), -2, "squeeze: use_part needs the partials output");
        const size_t n = (size_t)N * C * H * W;
        DevBuf x(in[0], n), aff(in[1], in[1] ? (size_t)C * 2 : 0), w(in[2], (size_t)C), epi(in[3], in[3] ? 2 : 0), z((size_t)N * H * W);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0];
        if (in[1]) t.aff0 = aff.p;
        const int nblk = launch_squeeze_conv(t, w.p, z.p, nullptr, true, st);
        DevBuf part((size_t)nblk * 2);
        launch_squeeze_conv(t, w.p, z.p, use_part ? part.p : nullptr, false, st, in[3] ? epi.p : nullptr);
        VR_HIP(hipStreamSynchronize(st));
        z.download(out[0]);
        if (use_part) part.download(out[1]);
        if (nout >= 3 && out[2]) out[2][0] = (float)nblk;
    } else if (name == "head_bwd") {
        need(4, 0, 2, 1);
        const int N = (int)dims[0], H = (int)dims[1], W = (int)dims[2], bins = (int)dims[3];
        VR_CHECK(N > 0 && H > 0 && W > 0 && bins >= H, -2, "head_bwd: need positive sizes and bins >= H");
        const size_t nm = (size_t)N * 2 * bins * W;
        DevBuf dmask(in[0], nm), mask(in[1], nm), dlogit((size_t)N * 2 * H * W);
        launch_head_bwd(dmask.p, mask.p, N, H, W, bins, dlogit.p, st);
        VR_HIP(hipStreamSynchronize(st));
        dlogit.download(out[0]);
    } else if (name == "crop") {
        need(5, 0, 2, 1);
        const long long rows = dims[0];
        const int T = (int)dims[1], Wm = (int)dims[2], off = (int)dims[3];
        const bool cplx = dims[4] != 0;
        VR_CHECK(rows > 0 && Wm > 0 && off >= 0 && off + Wm <= T, -2, "crop: need rows, Wm > 0 and 0 <= off, off + Wm <= T");
        const bool loss = !cplx && nin >= 3 && in[2] && nout >= 2 && out[1];
        const size_t E = cplx ? 2 : 1;
        DevBuf m(in[0], (size_t)rows * Wm * E), x(in[1], (size_t)rows * T * E), y(loss ? in[2] : nullptr, loss ? (size_t)rows * T : 0);
        DevBuf part((size_t)l1_crop_blocks()), lossd(4);
        launch_mul_crop(x.p, m.p, cplx, rows, T, Wm, off, st);
        if (loss) launch_l1_crop(L1_CROP_REAL, m.p, y.p, rows, T, Wm, off, part.p, lossd.p, st);
        VR_HIP(hipStreamSynchronize(st));
        m.download(out[0]);
        if (loss) VR_HIP(hipMemcpy(out[1], lossd.p, sizeof(float), hipMemcpyDeviceToHost));
    } else if (name == "rows") {
        need(3, 0, 3, 2);
        const int N = (int)dims[0], R = (int)dims[1], W = (int)dims[2];
        const size_t n = (size_t)N * R * W;
        DevBuf x(in[0], n), aff(in[1], (size_t)R * 2), d(in[2], n), o(n), sums(R);
        launch_rows_affine_relu(x.p, o.p, aff.p, N, R, W, st);
        launch_channel_sum(d.p, N, R, W, sums.p, 0, st);
        VR_HIP(hipStreamSynchronize(st));
        o.download(out[0]); sums.download(out[1]);
    } else if (name == "rows_gemm") {
        // dims: N, T, K, Cout, CoutPad, flags[, tile: 0 = the host's choice, 11 / 21 / 22].  in: x [N][K][T], w [K][CoutPad] (K-major, as stored), bias [Cout] or null, epi [Cout][2] or
        // null; fp[0]: activation slope behind epi.  out[0]: [N][Cout][T] of ONE launch_rows_gemm, between guard bands (-3); flags & 1:
        // out[1] = the same product as Model::run_lstm states it for run_conv (a 1x1 conv on the batch-as-rows view, launch_conv)
        need(6, 1, 2, 1);
        const int N = (int)dims[0], T = (int)dims[1], K = (int)dims[2], Cout = (int)dims[3], CoutPad = (int)dims[4];
        const bool conv_too = dims[5] & 1;
        VR_CHECK(N >= 1 && T >= 1 && K >= 1 && Cout >= 1 && CoutPad >= 1 && in[0] && in[1] && out[0], -2, "rows_gemm: sizes must be positive");
        VR_CHECK(!conv_too || (nout >= 2 && out[1] && CoutPad % 32 == 0 && CoutPad >= Cout), -2, "rows_gemm: the conv launch needs couts padded to 32 and out[1]");
        const size_t no = (size_t)N * Cout * T;
        DevBuf x(in[0], (size_t)N * K * T), w(in[1], (size_t)K * CoutPad);
        DevBuf bias(nin >= 3 ? in[2] : nullptr, nin >= 3 && in[2] ? (size_t)Cout : 0), epi(nin >= 4 ? in[3] : nullptr, nin >= 4 && in[3] ? (size_t)Cout * 2 : 0);
        const bool has_bias = nin >= 3 && in[2], has_epi = nin >= 4 && in[3];
        GuardedBuf o(out[0], no);                                 // (the caller's fill stays where the launch does not store)
        RowsGemmArgs g{};
        g.x = x.p; g.xN = (long long)K * T; g.w = w.p; g.bias = has_bias ? bias.p : nullptr; g.epi = has_epi ? epi.p : nullptr; g.slope = fp[0];
        g.out = o.p(); g.N = N; g.T = T; g.K = K; g.Cout = Cout; g.CoutPad = CoutPad;
        launch_rows_gemm(g, st, ndims >= 7 ? (int)dims[6] : 0);   // (refuses, -2, what rows_gemm_ok refuses and a tile it does not have)
        DevBuf oc(conv_too ? no : 0);
        if (conv_too) {
            ConvArgs a{};
            a.nsrc = 1; a.N = 1; a.Cin = K; a.c1 = a.c2 = K; a.Cout = Cout; a.CoutPad = CoutPad;
            a.d1 = a.d2 = 1 << 30;
            a.bf16 = mfma_mode;
            Tensor xt = dense(x.p, N, K, 1, T);
            a.src[0] = make_src(xt, false, 0);
            a.src[0].sH = a.src[0].sN; a.src[0].sN = 0; a.src[0].H = N;
            a.Hin = a.Hout = N; a.Win = a.Wout = T;
            a.w = w.p; a.bias = g.bias;
            if (has_epi) { a.epi = epi.p; a.epi_slope = fp[0]; }
            a.dst[0] = ConvDst{oc.p, 0, (long long)T, (long long)Cout * T, 0, 0};
            launch_conv(a, ConvShape{1, 1, 1, 1}, st);
        }
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(o.intact(), -3, "rows_gemm: a store outside the output buffer");
        o.download(out[0]);
        if (conv_too) oc.download(out[1]);
    } else if (name == "aspp_pool") {
        // dims: N, C8, H (W = 16).  in: x5 [N][C8][H][16], the pooled branch's 1x1 weights [C8][C8] and folded BatchNorm [C8][2], the four
        // branch convs' weights (1x1 [C8][C8], then three 3x3 [C8][C8][3][3] for dilation (4,2), (8,4), (12,6)) and their folded
        // BatchNorms [4][C8][2]; fp[0]: the pooled branch's activation slope.  An ASPP module's eval launches in mfma_mode 3, twice:
        //   out[0], out[1]: ONE group launch with the pooled branch as its fifth part -> f1 [N][C8][16] (between guard bands, over the
        //                   caller's fill) and the four branch outputs [N][4 C8][H][16]
        //   out[2], out[3]: launch_avgpool_h + the 1x1 conv as Model::run_conv states it (batch-as-rows, launch_conv) -> f1, and the group
        //                   launch without the fifth part -> the branch outputs
        need(3, 1, 8, 4);
        const int N = (int)dims[0], C8 = (int)dims[1], H = (int)dims[2], W = 16, CoutPad = (C8 + 31) / 32 * 32;
        VR_CHECK(N >= 1 && C8 >= 1 && H >= 1, -2, "aspp_pool: sizes must be positive");
        VR_CHECK(mfma_mode == 3, -2, "aspp_pool: the group launch runs in mfma_mode 3");
        for (int i = 0; i < 8; ++i) VR_CHECK(in[i] != nullptr, -2, "aspp_pool: missing input");
        const size_t nx = (size_t)N * C8 * H * W, nf = (size_t)N * C8 * W;
        DevBuf x(in[0], nx), epi1(in[2], (size_t)C8 * 2), epib(in[7], (size_t)4 * C8 * 2), cat_a(4 * nx), cat_b(4 * nx), pooled(nf), f1b(nf);
        GuardedBuf f1a(out[0], nf);
        const Tensor xt = dense(x.p, N, C8, H, W);
        std::vector<std::unique_ptr<DevBuf>> keep;
        auto kmajor = [&](const float* oihw, int KK) {
            std::vector<float> wk((size_t)C8 * KK * CoutPad, 0.f);
            for (int co = 0; co < C8; ++co)
                for (int ci = 0; ci < C8; ++ci)
                    for (int k = 0; k < KK; ++k) wk[((size_t)ci * KK + k) * CoutPad + co] = oihw[((size_t)co * C8 + ci) * KK + k];
            keep.emplace_back(new DevBuf(wk.data(), wk.size()));
            return keep.back()->p;
        };
        ConvArgs c4[4];
        ConvShape s4[4];
        LocalConv wf[4];
        for (int j = 0; j < 4; ++j) {
            const int KS = j ? 3 : 1, dh = j ? 4 * j : 1, dw = j ? 2 * j : 1;
            ConvArgs& a = c4[j];
            a = ConvArgs{};
            a.nsrc = 1; a.src[0] = make_src(xt, false, 0); a.c1 = a.c2 = a.Cin = C8;
            a.w = kmajor(in[3 + j], KS * KS); a.Cout = C8; a.CoutPad = CoutPad;
            a.epi = epib.p + (size_t)j * C8 * 2; a.epi_slope = 0.f;
            a.bf16 = 3; a.d1 = a.d2 = 1 << 30;
            a.N = N; a.Hin = a.Hout = H; a.Win = a.Wout = W; a.pad_h = j ? dh : 0; a.pad_w = j ? dw : 0;
            debug_weight_forms(a.w, C8, KS, 1, dh, dw, CoutPad, W, true, a, wf[j]);
            a.dst[0] = ConvDst{cat_a.p + (size_t)j * C8 * H * W, (long long)4 * C8 * H * W, (long long)H * W, W, 0, 0};
            s4[j] = ConvShape{KS, 1, dh, dw};
        }
        VR_CHECK(x3d_aspp_eligible(c4, s4), -2, "aspp_pool: conv_x3d does not take these four branch convs as one launch");
        X3dPoolArgs q{};
        q.x = x.p; q.xN = xt.sN; q.xC = xt.sC; q.xH = xt.sH;
        q.w = kmajor(in[1], 1); q.epi = epi1.p; q.slope = fp[0]; q.out = f1a.p();
        q.C8 = C8; q.H = H; q.Cout = C8; q.CoutPad = CoutPad;
        VR_CHECK(x3d_pool_eligible(q, c4), -2, "aspp_pool: the group launch cannot carry this pooled branch (x3d_pool_eligible)");
        x3d_launch_aspp(c4, st, &q);
        for (int j = 0; j < 4; ++j) c4[j].dst[0].p = cat_b.p + (size_t)j * C8 * H * W;
        launch_avgpool_h(xt, pooled.p, st);
        {
            ConvArgs b{};
            b.nsrc = 1; b.N = 1; b.Cin = C8; b.c1 = b.c2 = C8; b.Cout = C8; b.CoutPad = CoutPad;
            b.d1 = b.d2 = 1 << 30;
            b.bf16 = 3;
            b.src[0] = make_src(dense(pooled.p, N, C8, 1, W), false, 0);
            b.src[0].sH = b.src[0].sN; b.src[0].sN = 0; b.src[0].H = N;
            b.Hin = b.Hout = N; b.Win = b.Wout = W;
            b.w = q.w; b.epi = epi1.p; b.epi_slope = fp[0];
            b.dst[0] = ConvDst{f1b.p, 0, (long long)W, (long long)C8 * W, 0, 0};
            launch_conv(b, ConvShape{1, 1, 1, 1}, st);
        }
        x3d_launch_aspp(c4, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(f1a.intact(), -3, "aspp_pool: a store outside f1's buffer");
        f1a.download(out[0]); cat_a.download(out[1]); f1b.download(out[2]); cat_b.download(out[3]);
    } else if (name == "adam") {
        need(1, 6, 4, 3);
        const size_t n = (size_t)dims[0];
        // the float parameters arrive as fp32; snap them back to the decimal doubles the optimizer was built with
        double dp[6];
        for (int i = 0; i < 6; ++i) {
            char buf[48];
            std::snprintf(buf, sizeof buf, "%.7g", (double)fp[i]);
            dp[i] = std::strtod(buf, nullptr);
        }
        DevBuf p(in[0], n), g(in[1], n), m(in[2], n), v(in[3], n);
        launch_adam(p.p, g.p, m.p, v.p, (long long)n, dp[0], dp[1], dp[2], dp[3], (long long)dp[5], dp[4], st);
        VR_HIP(hipStreamSynchronize(st));
        p.download(out[0]); m.download(out[1]); v.download(out[2]);
    } else if (name == "stream_post") {
        need(2, 0, 1, 2);
        const int T = (int)dims[0], n_cuts = ndims - 2;
        VR_CHECK(T > 0 && in[0] && out[0] && out[1], -2, "stream_post: need T > 0, the minima and two outputs");
        int step = 0;
        for (int k = 0, at = 0; k <= n_cuts; ++k) {
            const int to = k < n_cuts ? (int)dims[2 + k] : T;
            VR_CHECK(to >= at && to <= T && to > 0, -2, "stream_post: cuts must ascend inside (0, T]");
            step = std::max(step, to - at);
            at = to;
        }
        const int RW = dims[1] ? (int)dims[1] : kStreamPostDelay + step;
        VR_CHECK(RW >= kStreamPostDelay + step, -2, "stream_post: the ring must hold 161 + the largest step");
        GuardedBuf fring(nullptr, (size_t)RW), wring(nullptr, (size_t)RW);
        DevBuf state(8), table((sizeof(StreamSeg) + 3) / 4);
        VR_HIP(hipMemset(fring.p(), 0, (size_t)RW * 4));
        VR_HIP(hipMemset(wring.p(), 0, (size_t)RW * 4));
        VR_HIP(hipDeviceSynchronize());
        std::vector<float> host_ring((size_t)RW, 0.f);
        int final_n = 0;
        auto declare = [&](int n) {
            if (n <= final_n) return;
            VR_HIP(hipMemcpy(host_ring.data(), wring.p(), (size_t)RW * 4, hipMemcpyDeviceToHost));
            for (; final_n < n; ++final_n) out[0][final_n] = host_ring[(size_t)(final_n % RW)];
        };
        for (int k = 0, at = 0; k <= n_cuts; ++k) {
            const int to = k < n_cuts ? (int)dims[2 + k] : T;
            for (int t = at; t < to; ++t) VR_HIP(hipMemcpy(fring.p() + t % RW, in[0] + t, 4, hipMemcpyHostToDevice));
            StreamSeg g{};
            g.fmin_ring = fring.p(); g.wgt_ring = wring.p(); g.post = reinterpret_cast<StreamPostState*>(state.p); g.RW = RW;
            g.fm_lo = at; g.fm_hi = to; g.post_flush = k == n_cuts;
            VR_HIP(hipMemcpy(table.p, &g, sizeof g, hipMemcpyHostToDevice));
            launch_stream_post(reinterpret_cast<const StreamSeg*>(table.p), 1, 0, (double)(to - at), true, false, false, n_fft / 2 + 1, st);
            VR_HIP(hipStreamSynchronize(st));
            if (k < n_cuts) {
                declare(std::max(0, to - kStreamPostDelay));
                out[1][k] = (float)final_n;
            }
            at = to;
        }
        declare(T);
        out[1][n_cuts] = (float)final_n;
        VR_CHECK(fring.intact() && wring.intact(), -3, "stream_post: a store outside a ring");
        if (nout >= 3 && out[2]) wring.download(out[2]);
    } else if (name == "wire") {
        need(1, 0, 1, 1);
        const size_t n = (size_t)dims[0];
        DevBuf x(in[0], n), half((n + 1) / 2), y(n);
        launch_f32_to_bf16(x.p, reinterpret_cast<unsigned short*>(half.p), (long long)n, st);
        launch_bf16_to_f32(reinterpret_cast<const unsigned short*>(half.p), y.p, (long long)n, st);
        VR_HIP(hipStreamSynchronize(st));
        y.download(out[0]);
    } else if (name == "signal_norm") {
        need(6, 0, 1, 2);
        const int bins = (int)dims[0], T = (int)dims[1], Wpad = (int)dims[2], pad_l = (int)dims[3], mode = (int)dims[4];
        const bool cplx = dims[5] != 0;
        VR_CHECK(bins > 0 && T > 0 && pad_l >= 0 && Wpad >= pad_l + T, -2, "signal_norm: need bins, T > 0 and Wpad >= pad_l + T");
        const size_t nmag = (size_t)(cplx ? 4 : 2) * bins * Wpad;
        // the magnitude path zeroes its crop source first; the complex pack writes every column itself, so it starts from NaN here
        std::vector<float> fill(nmag, cplx ? std::nanf("") : 0.f);
        DevBuf spec(in[0], (size_t)2 * bins * T * 2), mag(fill.data(), nmag), stats(4 + (size_t)2 * bins * 4), aff(4);
        unsigned* sp = reinterpret_cast<unsigned*>(stats.p);
        launch_mag_pad(reinterpret_cast<const float2*>(spec.p), bins, T, mag.p, Wpad, pad_l, sp, st);
        if (cplx) {
            launch_coef_complex(sp, 2 * bins, mode, reinterpret_cast<float2*>(aff.p), st);
            launch_pack_complex(reinterpret_cast<const float2*>(spec.p), 1, bins, T, mag.p, Wpad, pad_l, reinterpret_cast<const float2*>(aff.p), st);
        } else {
            launch_coef_affine(sp, 2 * bins, mode, aff.p, st);
        }
        VR_HIP(hipStreamSynchronize(st));
        mag.download(out[0]); aff.download(out[1]);
        if (nout >= 3 && out[2]) VR_HIP(hipMemcpy(out[2], stats.p, 4 * sizeof(float), hipMemcpyDeviceToHost));
    } else if (name == "signal_mask") {
        need(7, 0, 4, 3);
        const int T = (int)dims[0], Wa = (int)dims[1], Wb = (int)dims[2], shift = (int)dims[3];
        const bool has_b = dims[4] != 0, has_wgt = dims[5] != 0, cplx = dims[6] != 0;
        const int bins = n_fft / 2 + 1;
        VR_CHECK(T > 0 && Wa >= T && (!has_b || (shift >= 0 && Wb >= T + shift)), -2, "signal_mask: the masks must cover T (+ shift) frames");
        VR_CHECK(in[0] && in[1] && (!has_b || in[2]) && (!has_wgt || in[3]), -2, "signal_mask: missing input");
        const size_t rows = (size_t)2 * bins, mc = cplx ? 2 : 1, nspec = rows * T * 2, nwave = (size_t)2 * hop * (T - 1);
        DevBuf spec(in[0], nspec), ma(in[1], rows * Wa * mc), mb(has_b ? in[2] : nullptr, has_b ? rows * Wb * mc : 0);
        DevBuf wgt(has_wgt ? in[3] : nullptr, has_wgt ? (size_t)T : 0);
        DevBuf fmin((size_t)T), y(nspec), v(nspec), yw(nwave), vw(nwave);
        const float2* sd = reinterpret_cast<const float2*>(spec.p);
        const float* mbp = has_b ? mb.p : nullptr;
        const float* wp = has_wgt ? wgt.p : nullptr;
        const bool waves = nout >= 5 && out[3] && out[4];
        VR_CHECK(!waves || istft_masked_available(plan, hop), -2, "signal_mask: the fused masked iSTFT needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        if (cplx) {
            const float2 *a2 = reinterpret_cast<const float2*>(ma.p), *b2 = reinterpret_cast<const float2*>(mbp);
            launch_frame_min_complex(bins, T, a2, Wa, b2, Wb, shift, fmin.p, st);
            launch_apply_mask_complex(sd, bins, T, a2, Wa, b2, Wb, shift, wp, reinterpret_cast<float2*>(y.p), reinterpret_cast<float2*>(v.p), st);
            if (waves)
                for (int which = 0; which < 2; ++which)
                    launch_istft_masked_complex(plan, sd, hop, T, a2, Wa, b2, Wb, shift, wp, which, which ? vw.p : yw.p, st);
        } else {
            launch_frame_min(bins, T, ma.p, Wa, mbp, Wb, shift, fmin.p, st);
            launch_apply_mask(sd, bins, T, ma.p, Wa, mbp, Wb, shift, wp, reinterpret_cast<float2*>(y.p), reinterpret_cast<float2*>(v.p), st);
            if (waves)
                for (int which = 0; which < 2; ++which)
                    launch_istft_masked(plan, sd, hop, T, ma.p, Wa, mbp, Wb, shift, wp, which, which ? vw.p : yw.p, st);
        }
        VR_HIP(hipStreamSynchronize(st));
        fmin.download(out[0]); y.download(out[1]); v.download(out[2]);
        if (waves) { yw.download(out[3]); vw.download(out[4]); }
    } else if (name == "wave_eval") {
        need(10, 0, 6, 4);
        const int T = (int)dims[0], Wa = (int)dims[1], Wb = (int)dims[2], shift = (int)dims[3];
        const bool has_b = dims[4] != 0, has_wgt = dims[5] != 0, cplx = dims[6] != 0, store = dims[8] != 0;
        const long long window = dims[7], L = dims[9];
        const int bins = n_fft / 2 + 1;
        VR_CHECK(many_tiled_available(plan, hop), -2, "wave_eval: the evaluation form needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        VR_CHECK(T >= 2 && Wa >= T && (!has_b || (shift >= 0 && Wb >= T + shift)), -2, "wave_eval: need T >= 2 and masks that cover T (+ shift) frames");
        VR_CHECK(window >= hop && L >= (long long)hop * (T - 1), -2, "wave_eval: need window >= hop and L >= hop (T-1)");
        VR_CHECK(in[0] && in[1] && (!has_b || in[2]) && (!has_wgt || in[3]) && in[4] && in[5], -2, "wave_eval: missing input");
        const size_t rows = (size_t)2 * bins, mc = cplx ? 2 : 1, nspec = rows * T * 2, nwave = (size_t)2 * hop * (T - 1);
        const long long samples = (long long)hop * (T - 1), windows = (samples + window - 1) / window;
        DevBuf spec(in[0], nspec), ma(in[1], rows * Wa * mc), mb(has_b ? in[2] : nullptr, has_b ? rows * Wb * mc : 0);
        DevBuf wgt(has_wgt ? in[3] : nullptr, has_wgt ? (size_t)T : 0), mix(in[4], (size_t)2 * L), inst(in[5], (size_t)2 * L);
        GuardedBuf yw(nullptr, nwave), vw(nullptr, nwave), part(nullptr, 2 * eval_part_doubles(T)), sums(nullptr, (size_t)windows * 8);
        DevBuf table((sizeof(SongSeg) + 3) / 4), entry((sizeof(WaveEval) + 3) / 4);
        SongSeg sg{};
        sg.wave = mix.p; sg.L = L; sg.spec = reinterpret_cast<float2*>(spec.p); sg.y_wave = yw.p(); sg.v_wave = vw.p(); sg.T = T;
        WaveEval ev{};
        ev.inst = inst.p; ev.part = reinterpret_cast<double*>(part.p()); ev.sums = reinterpret_cast<double*>(sums.p());
        ev.window = window; ev.store = store ? 1 : 0;
        VR_HIP(hipMemcpy(table.p, &sg, sizeof(SongSeg), hipMemcpyHostToDevice));
        VR_HIP(hipMemcpy(entry.p, &ev, sizeof(WaveEval), hipMemcpyHostToDevice));
        const SongSeg* tab = reinterpret_cast<const SongSeg*>(table.p);
        const WaveEval* evd = reinterpret_cast<const WaveEval*>(entry.p);
        for (int which = 0; which < 2; ++which)
            launch_istft_eval_many(plan, tab, evd, 1, T, (double)T, ma.p, Wa, has_b ? mb.p : nullptr, Wb, shift, cplx, has_wgt ? wgt.p : nullptr, which,
                                   store, st);
        launch_eval_sums(plan, tab, evd, 1, windows, (double)T, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(yw.intact() && vw.intact() && part.intact() && sums.intact(), -3, "wave_eval: a store outside a stem, the partial sums or the sums");
        yw.download(out[0]); vw.download(out[1]); sums.download(out[2]);
        if (out[3]) { out[3][0] = (float)eval_tile_step(plan); out[3][1] = (float)windows; }
    } else if (name == "wave_pair") {
        need(6, 0, 3, 3);
        const int S = (int)dims[0], T = (int)dims[1], xp = (int)dims[2], yp = (int)dims[3], yo = (int)dims[4];
        const bool has_mask = dims[5] != 0;
        const int bins = n_fft / 2 + 1;
        VR_CHECK(wave_loss_available(plan, hop), -2, "wave_pair: the pair iSTFT needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        VR_CHECK(S > 0 && T >= 2 && xp >= T && yo >= 0 && yp >= yo + T && in[0] && in[2] && (!has_mask || in[1]), -2,
                 "wave_pair: need signals > 0, T >= 2, x_pitch >= T, y_pitch >= y_off + T and the inputs");
        const size_t rows = (size_t)S * bins, nw = (size_t)S * hop * (T - 1);
        const WaveTermFloats wf = wave_term_floats(plan, hop, 1, S, T);
        DevBuf x(in[0], rows * xp * 2), m(has_mask ? in[1] : nullptr, has_mask ? rows * xp * 2 : 0), y(in[2], rows * yp * 2);
        GuardedBuf yw(nullptr, nw), pw(nullptr, nw), part(nullptr, wf.part);
        DevBuf sums(4), table(wf.table);
        WavePair pr{};
        pr.x = reinterpret_cast<const float2*>(x.p); pr.mask = has_mask ? reinterpret_cast<const float2*>(m.p) : nullptr;
        pr.y = reinterpret_cast<const float2*>(y.p); pr.x_pitch = xp; pr.y_pitch = yp; pr.y_off = yo;
        pr.y_wave = yw.p(); pr.p_wave = pw.p(); pr.part = part.p();
        launch_wave_term(plan, pr, table.p, nullptr, S, T, sums.p, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(yw.intact() && pw.intact() && part.intact(), -3, "wave_pair: a store outside a wave or the partial sums");
        yw.download(out[0]); pw.download(out[1]);
        VR_HIP(hipMemcpy(out[2], sums.p, 3 * sizeof(float), hipMemcpyDeviceToHost));
    } else if (name == "wave_grad") {
        need(3, 2, 6, 1);
        const int S = (int)dims[0], T = (int)dims[1];
        const bool l1 = dims[2] != 0;
        const int bins = n_fft / 2 + 1;
        VR_CHECK(wave_loss_available(plan, hop), -2, "wave_grad: the gradient STFT needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        VR_CHECK(S > 0 && T >= 2 && in[0] && in[1] && in[2] && in[3] && (!l1 || (in[4] && in[5])), -2, "wave_grad: need signals > 0, T >= 2 and the inputs");
        const size_t ns = (size_t)S * bins * T * 2, nw = (size_t)S * hop * (T - 1);
        DevBuf yw(in[0], nw), pw(in[1], nw), sums(in[2], 3), X(in[3], ns), m(l1 ? in[4] : nullptr, l1 ? ns : 0), Y(l1 ? in[5] : nullptr, l1 ? ns : 0);
        GuardedBuf dm(nullptr, ns);
        WaveGrad g{};
        g.y_wave = yw.p; g.p_wave = pw.p; g.sums = sums.p; g.X = reinterpret_cast<const float2*>(X.p);
        g.mask = reinterpret_cast<const float2*>(m.p); g.Y = reinterpret_cast<const float2*>(Y.p);
        g.dmask = reinterpret_cast<float2*>(dm.p()); g.sdr_scale = fp[0]; g.l1_scale = l1 ? fp[1] : 0.f;
        launch_stft_wave_grad(plan, g, S, T, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(dm.intact(), -3, "wave_grad: a store outside dmask");
        dm.download(out[0]);
    } else if (name == "head_wave_loss") {
        need(5, 3, 5, 6);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3], bins = (int)dims[4];
        const bool head_only = ndims >= 6 && dims[5] != 0;
        VR_CHECK(head_only || (wave_loss_available(plan, hop) && bins == n_fft / 2 + 1), -2,
                 "head_wave_loss: bins must be n_fft / 2 + 1 of a hop == n_fft / 2 handle (or head_only)");
        VR_CHECK(N > 0 && C > 0 && H > 0 && W >= 2 && bins >= H && W % 4 == 0, -2, "head_wave_loss: need positive sizes, bins >= H, W % 4 == 0");
        const size_t n = (size_t)N * C * H * W, nx = (size_t)N * 2 * bins * W;
        const WaveTermFloats wf = head_only ? WaveTermFloats{} : wave_term_floats(plan, hop, 1, N * 2, W);
        DevBuf x(in[0], n), aff(in[1], in[1] ? (size_t)C * 2 : 0), w(in[2], (size_t)4 * C), X(in[3], 2 * nx), Y(in[4], 2 * nx);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0];
        if (in[1]) t.aff0 = aff.p;
        DevBuf dlogit((size_t)N * 4 * H * W), mask(2 * nx), lpart((size_t)head_loss_blocks(t)), loss(4), g(n), dw((size_t)4 * C);
        DevBuf part((size_t)thin_wgrad_blocks(t) * 4 * C), yw(wf.wave), pw(wf.wave), pp(wf.part), dm(2 * nx), table(64);
        const HeadScratch hs{dlogit.p, lpart.p, part.p, nullptr, dm.p, {yw.p, pw.p, nullptr}, pp.p, table.p};
        run_train_head(plan, t, TrainHead{1, true, w.p, X.p, Y.p, bins, mask.p, loss.p, (float)(1.0 / (double)nx), fp[2], fp[1], head_only ? nullptr : g.p, 0,
                                          head_only ? nullptr : dw.p, 0}, hs, nullptr, st);
        VR_HIP(hipStreamSynchronize(st));
        if (head_only) {
            mask.download(out[1]);
            VR_HIP(hipMemcpy(out[2], loss.p, 4 * sizeof(float), hipMemcpyDeviceToHost));
            return;
        }
        dlogit.download(out[0]); mask.download(out[1]);
        VR_HIP(hipMemcpy(out[2], loss.p, 4 * sizeof(float), hipMemcpyDeviceToHost));
        g.download(out[3]); dw.download(out[4]); dm.download(out[5]);
    } else if (name == "wave_triple") {
        need(6, 0, 4, 4);
        const int S = (int)dims[0], T = (int)dims[1], xp = (int)dims[2], xo = (int)dims[3], pp = (int)dims[4];
        const bool has_mask = dims[5] != 0;
        const int bins = n_fft / 2 + 1;
        VR_CHECK(wave_loss_available(plan, hop), -2, "wave_triple: the triple iSTFT needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        VR_CHECK(S > 0 && T >= 2 && xo >= 0 && xp >= xo + T && in[0] && in[1] && (has_mask ? in[2] != nullptr : (in[3] && pp >= T)), -2,
                 "wave_triple: need signals > 0, T >= 2, xy_pitch >= xy_off + T, the inputs, and a mask or an estimate with p_pitch >= T");
        const size_t rows = (size_t)S * bins, nw = (size_t)S * hop * (T - 1);
        const WaveTermFloats wf = wave_term_floats(plan, hop, 3, S, T);
        DevBuf x(in[0], rows * xp * 2), y(in[1], rows * xp * 2), m(has_mask ? in[2] : nullptr, has_mask ? rows * xp * 2 : 0);
        DevBuf pe(has_mask ? nullptr : in[3], has_mask ? 0 : rows * pp * 2);
        GuardedBuf xw(nullptr, nw), yw(nullptr, nw), pw(nullptr, nw), part(nullptr, wf.part), sums(nullptr, 6);
        DevBuf table(wf.table);
        WaveTriple tr{};
        tr.x = reinterpret_cast<const float2*>(x.p); tr.y = reinterpret_cast<const float2*>(y.p);
        tr.mask = has_mask ? reinterpret_cast<const float2*>(m.p) : nullptr; tr.p = has_mask ? nullptr : reinterpret_cast<const float2*>(pe.p);
        tr.xy_pitch = xp; tr.xy_off = xo; tr.p_pitch = has_mask ? xp : pp;
        tr.x_wave = xw.p(); tr.y_wave = yw.p(); tr.p_wave = pw.p(); tr.part = part.p();
        launch_wave_term(plan, tr, table.p, nullptr, S, T, sums.p(), st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(xw.intact() && yw.intact() && pw.intact() && part.intact() && sums.intact(), -3,
                 "wave_triple: a store outside a wave, the partial sums or the sums");
        xw.download(out[0]); yw.download(out[1]); pw.download(out[2]); sums.download(out[3]);
    } else if (name == "wave_grad3") {
        need(3, 2, 7, 1);
        const int S = (int)dims[0], T = (int)dims[1];
        const bool l1 = dims[2] != 0;
        const int bins = n_fft / 2 + 1;
        VR_CHECK(wave_loss_available(plan, hop), -2, "wave_grad3: the gradient STFT needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        VR_CHECK(S > 0 && T >= 2 && in[0] && in[1] && in[2] && in[3] && in[4] && (!l1 || (in[5] && in[6])), -2,
                 "wave_grad3: need signals > 0, T >= 2 and the inputs");
        const size_t ns = (size_t)S * bins * T * 2, nw = (size_t)S * hop * (T - 1);
        DevBuf xw(in[0], nw), yw(in[1], nw), pw(in[2], nw), sums(in[3], 6), X(in[4], ns), m(l1 ? in[5] : nullptr, l1 ? ns : 0),
            Y(l1 ? in[6] : nullptr, l1 ? ns : 0);
        GuardedBuf dm(nullptr, ns);
        WaveGrad3 g{};
        g.x_wave = xw.p; g.y_wave = yw.p; g.p_wave = pw.p; g.sums = sums.p; g.X = reinterpret_cast<const float2*>(X.p);
        g.mask = reinterpret_cast<const float2*>(m.p); g.Y = reinterpret_cast<const float2*>(Y.p);
        g.dmask = reinterpret_cast<float2*>(dm.p()); g.sdr_scale = fp[0]; g.l1_scale = l1 ? fp[1] : 0.f;
        launch_stft_wave_grad3(plan, g, S, T, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(dm.intact(), -3, "wave_grad3: a store outside dmask");
        dm.download(out[0]);
    } else if (name == "head_wave_wsdr") {
        need(5, 3, 5, 6);
        const int N = (int)dims[0], C = (int)dims[1], H = (int)dims[2], W = (int)dims[3], bins = (int)dims[4];
        VR_CHECK(wave_loss_available(plan, hop) && bins == n_fft / 2 + 1, -2, "head_wave_wsdr: bins must be n_fft / 2 + 1 of a hop == n_fft / 2 handle");
        VR_CHECK(N > 0 && C > 0 && H > 0 && W >= 2 && bins >= H && W % 4 == 0, -2, "head_wave_wsdr: need positive sizes, bins >= H, W % 4 == 0");
        const size_t n = (size_t)N * C * H * W, nx = (size_t)N * 2 * bins * W;
        const WaveTermFloats wf = wave_term_floats(plan, hop, 3, N * 2, W);
        DevBuf x(in[0], n), aff(in[1], in[1] ? (size_t)C * 2 : 0), w(in[2], (size_t)4 * C), X(in[3], 2 * nx), Y(in[4], 2 * nx);
        Tensor t = dense(x.p, N, C, H, W);
        t.slope = fp[0];
        if (in[1]) t.aff0 = aff.p;
        DevBuf dlogit((size_t)N * 4 * H * W), mask(2 * nx), lpart((size_t)head_loss_blocks(t)), g(n), dw((size_t)4 * C);
        DevBuf part((size_t)thin_wgrad_blocks(t) * 4 * C), table(wf.table);
        GuardedBuf loss(nullptr, 7), xw(nullptr, wf.wave), yw(nullptr, wf.wave), pw(nullptr, wf.wave), pp(nullptr, wf.part), dm(nullptr, 2 * nx);
        const HeadScratch hs{dlogit.p, lpart.p, part.p, nullptr, dm.p(), {yw.p(), pw.p(), xw.p()}, pp.p(), table.p};
        run_train_head(plan, t, TrainHead{3, true, w.p, X.p, Y.p, bins, mask.p, loss.p(), (float)(1.0 / (double)nx), fp[2], fp[1], g.p, 0, dw.p, 0}, hs,
                       nullptr, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(loss.intact() && xw.intact() && yw.intact() && pw.intact() && pp.intact() && dm.intact(), -3,
                 "head_wave_wsdr: a store outside the loss, a wave, the partial sums or dmask");
        dlogit.download(out[0]); mask.download(out[1]); loss.download(out[2]); g.download(out[3]); dw.download(out[4]); dm.download(out[5]);
    } else if (name == "stft_crops") {
        need(3, 0, 1, 1);
        const int W = (int)dims[0], E = (int)dims[1], max_T = (int)dims[2];
        const int bins = n_fft / 2 + 1;
        VR_CHECK(many_tiled_available(plan, hop), -2, "stft_crops: the crop form needs hop == n_fft / 2 (128 <= n_fft <= 4096)");
        VR_CHECK(W > 0 && E > 0 && E <= 65535 && max_T > 0 && ndims >= 3 + 3 * W + 3 * E && nin >= W, -2,
                 "stft_crops: need waves, entries and max_T > 0 and three dims for every wave and every entry");
        std::vector<std::unique_ptr<DevBuf>> wv;
        for (int w = 0; w < W; ++w) {
            const long long n = dims[3 + 3 * w], fmt = dims[4 + 3 * w], chn = dims[5 + 3 * w];
            VR_CHECK(n > 0 && in[w] && (fmt == 0 || (fmt >= 1 && fmt <= 4 && (chn == 1 || chn == 2))), -2,
                     "stft_crops: wave " + std::to_string(w) + ": need n > 0, the samples, and fmt 0 or a vr_pcm_format with 1 or 2 channels");
            const size_t bytes = fmt == 0 ? (size_t)2 * n * 4 : (size_t)n * chn * (fmt == 1 ? 2 : fmt == 2 ? 3 : 4);
            wv.emplace_back(new DevBuf(in[w], (bytes + 3) / 4));
        }
        const size_t rows_f = (size_t)max_T * 2 * bins * 2;
        GuardedBuf rows(nullptr, (size_t)E * rows_f);
        std::vector<CropSeg> segs((size_t)E);
        int longest = 0;
        double rows_total = 0.0;
        for (int e = 0; e < E; ++e) {
            const int64_t* d = dims + 3 + 3 * W + 3 * e;
            VR_CHECK(d[0] >= 0 && d[0] < W, -2, "stft_crops: entry " + std::to_string(e) + ": wave index out of range");
            const long long n = dims[3 + 3 * d[0]], song_rows = 1 + n / hop;
            VR_CHECK(d[2] > 0 && d[2] <= max_T && d[1] >= 0 && d[1] <= song_rows - d[2], -2,
                     "stft_crops: entry " + std::to_string(e) + ": rows [" + std::to_string(d[1]) + ", " + std::to_string(d[1] + d[2]) +
                         ") must lie inside the " + std::to_string(song_rows) + " rows of its wave and T inside max_T");
            segs[e] = CropSeg{wv[d[0]]->p, n, d[1], reinterpret_cast<float2*>(rows.p() + (size_t)e * rows_f), (int)d[2], (int)dims[4 + 3 * d[0]],
                              (int)dims[5 + 3 * d[0]], 0};
            longest = std::max(longest, (int)d[2]);
            rows_total += (double)d[2];
        }
        DevBuf table(((size_t)E * sizeof(CropSeg) + 3) / 4);
        VR_HIP(hipMemcpy(table.p, segs.data(), (size_t)E * sizeof(CropSeg), hipMemcpyHostToDevice));
        launch_stft_crops(plan, reinterpret_cast<const CropSeg*>(table.p), E, longest, rows_total, st);
        VR_HIP(hipStreamSynchronize(st));
        VR_CHECK(rows.intact(), -3, "stft_crops: a store outside the scratch rows");
        rows.download(out[0]);
    } else {
        throw Error(-2, "vr_debug_kernel: unknown kernel name: " + name);
    }
}

}  // namespace vr
