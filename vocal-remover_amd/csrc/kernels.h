// Launch wrappers for the non-MFMA kernels of libvr_mi355.so (definitions in *.hip).
#pragma once
#include "stream_post.h"
#include "vr_common.h"

namespace vr {

// ---- pointwise.hip -----------------------------------------------------------------------------
// Thin-output 1x1 convs that are HBM-bound (Cout = 1 or 2): the LSTM squeeze conv
// (lib/layers.py:112) and the mask head `out` + sigmoid + replicate-pad + offset crop
// (lib/nets.py:79,109-115,127-128).
struct HeadDst {
    float* p;                 // destination base
    long long dN, dC, dH;     // strides of the destination (elements)
    int w_lo, w_hi;           // keep input columns [w_lo, w_hi); column w lands at w - w_lo
    int pad_rows;             // replicate the last input row this many extra times (1025 - 1024)
    // optional (mask heads only): a device table with one destination per batch item, used in place of p + n * dN -- the items of a
    // batch may then land in different buffers (Model::stream_run, for one stream as for many: one mask ring per stream and pass,
    // a crop's columns anywhere in it).  item_pitch[n] is then the
    // row pitch of item n's buffer, in place of dH, and rows * item_pitch[n] its plane pitch, in place of dC.
    float* const* items;
    const int* item_pitch;
};
void launch_head_sigmoid(const Tensor& x, const float* w /*[2][C]*/, const HeadDst& d, hipStream_t st);
// complex-mask head (is_complex, lib/nets.py:104-107,119-122): 4 outputs, m = complex(out[o], out[o+2]) for o = 0, 1, bounded as
// tanh(|m|) * m / (|m| + 1e-8); d.p holds complex64 and its strides count complex elements
void launch_head_complex(const Tensor& x, const float* w /*[4][C]*/, const HeadDst& d, hipStream_t st);
// out[n][0][h][w] = sum_c w[c] * act(x);  part: [nblocks][2] (sum, sumsq) or null; returns nblocks
// epi (eval): device [2] = folded (scale, shift) of the single-channel BatchNorm, applied with the ReLU before the store
int launch_squeeze_conv(const Tensor& x, const float* w /*[C]*/, float* out, float* part, bool dry, hipStream_t st,
                        const float* epi = nullptr);

// mean over H of act(x) -> out [N][C][W]  (AdaptiveAvgPool2d((1, None)), lib/layers.py:72)
void launch_avgpool_h(const Tensor& x, float* out, hipStream_t st);

// BatchNorm bookkeeping ---------------------------------------------------------------------------
struct BNFoldDesc { const float *w, *b, *rm, *rv; float* affine; int C; int bcast; };  // bcast>0: C==1, replicate to bcast rows
void launch_bn_fold_eval(const BNFoldDesc* d_descs, int ndesc, int maxC, float eps, hipStream_t st);
struct BNFinalizeArgs {
    const float* part; int nparts; int pstride;   // partial rows: part[i*pstride + c*2 + {0,1}]
    double count;                                  // elements per channel
    const float *w, *b; float *rm, *rv;           // running stats updated in place (momentum)
    float* affine; float* save_mean; float* save_invstd;
    int C; float eps, momentum;
    int broadcast;                                 // >0: C==1 stats, affine replicated to `broadcast` rows
};
void launch_bn_finalize(const BNFinalizeArgs& a, hipStream_t st);

// in-place rows affine + relu on [N][R][W]: v = relu(v*aff[r][0] + aff[r][1])  (BatchNorm1d + ReLU
// of lib/layers.py:120-121 applied to the Linear output laid out [N, nbins, nframes])
void launch_rows_affine_relu(const float* x, float* out, const float* aff, int N, int R, int W, hipStream_t st);

// out[i] = a[i] + b[i]
void launch_add(const float* a, const float* b, float* out, int n, hipStream_t st);

// dense post-activation copy of a Tensor (debug taps / tests)
void launch_materialize(const Tensor& x, float* out, hipStream_t st);
// training input pipeline (augment.hip); layout-compatible with vr_aug in include/vr_mi355.h
struct AugDesc { float coef, coef_mix, lam; int flags; };
void launch_augment(const float2* X, const float2* Y, const float2* Xi, const float2* Yi, const AugDesc* desc, const float* rw,
                    int B, int T, int bins, float* Xmag, float* Ymag, bool out_complex, hipStream_t st);
// (out_complex: the augmented x, y themselves as complex64 [B][2][bins][T] instead of their magnitudes -- a complex-mask model's batches)
// the same kernel reading the crops where they lie in a resident store: one entry per sample, every pointer at the sample's
// first row of its song's [rows][2][bins] slab (the mixup pair repeats the first two when the sample has no partner)
struct AugCrops { const float2 *X, *y, *X_mix, *y_mix; };
void launch_augment_resident(const AugCrops* table, const AugDesc* desc, const float* rw, int B, int T, int bins, float* Xmag,
                             float* Ymag, bool out_complex, hipStream_t st);
// the extended descriptor (vr_aug_ex): AugDesc's four fields and the two gains of a remix.  Flag bits beyond
// AugDesc's 0-6: kAugRemix (the partner is a remix partner: X = g_y y + g_v (X_j - y_j), y = g_y y), kAugMono (both channels become
// 0.5f * (L + R)) and kAugMixMono (the same for a mixup partner).  The two launchers above instantiated with it: same grid, same tile,
// same four crops a sample.
struct AugDescEx { float coef, coef_mix, lam; int flags; float gain_y, gain_v; };
constexpr int kAugMix = 8, kAugRemix = 128, kAugMono = 256, kAugMixMono = 512, kAugExBits = kAugRemix | kAugMono | kAugMixMono;
void launch_augment(const float2* X, const float2* Y, const float2* Xi, const float2* Yi, const AugDescEx* desc, const float* rw,
                    int B, int T, int bins, float* Xmag, float* Ymag, bool out_complex, hipStream_t st);
void launch_augment_resident(const AugCrops* table, const AugDescEx* desc, const float* rw, int B, int T, int bins, float* Xmag,
                             float* Ymag, bool out_complex, hipStream_t st);
// windows of resident songs (vr_dataset_windows): one entry per sample, the pointers at row 0 of the song's slabs;
// sample b is rows [start, start + T) of them, a row outside [0, rows) zero, every value read times `scale`
struct SongWindow { const float2 *X, *y; long long rows, start; float scale; int reserved; };
struct SongWindows { const SongWindow* table; int T, bins; float *X_out, *y_out; };      // outputs [B][2][bins][T], fp32 or complex64
void launch_song_windows(const SongWindow* table, int B, int T, int bins, float* X_out, float* y_out, bool out_complex, hipStream_t st);
// np.abs of one complex64 as numpy computes it (its loop for complex absolute, numpy 1.25 and later on a CPU with fused multiply-add):
// larger * sqrt(fma(ratio, ratio, 1)), ratio = smaller / larger, all float32 -- NOT hypotf, from which it differs in the last bit of
// about a third of all values, and not monotone in the exact magnitude.  Five correctly rounded IEEE operations: host and device agree.
__host__ __device__ inline float numpy_cabsf(float re, float im) {
    re = fabsf(re); im = fabsf(im);
    if (re == INFINITY || im == INFINITY) return INFINITY; // inf beside NaN is inf
    if (re != re || im != im) return NAN;
    const float larger = fmaxf(re, im), smaller = fminf(re, im);
    const float ratio = larger == 0.f ? 0.f : smaller / larger;
    return sqrtf(fmaf(ratio, ratio, 1.f)) * larger;
}
// the element of largest np.abs of one resident song (vr_dataset_peak): X, y slabs of n complex64 each (n even).  ws holds
// kPeakParts + 1 candidates: one per workgroup of the first launch, and at [song_peak_parts(n)] the result -- pos = the element's index
// in the sequence [X | y], key = its numpy_cabsf, bad = a NaN key was met, re, im = the element.
struct PeakCand { unsigned long long pos; float key; unsigned bad; float re, im; };
struct SongPeak { const float2 *X, *y; long long n; PeakCand* part; int parts; };
constexpr int kPeakParts = 2048;                          // 256 CUs x 8 workgroups; a shorter song launches fewer (song_peak_parts)
int song_peak_parts(long long n);
void launch_song_peak(const float2* X, const float2* y, long long n, PeakCand* ws, hipStream_t st);
// the pitch forms of the same kernel family: the argument struct selects the body
struct PitchDiff { const float* mix; const float* inst; float* v; long long n; };          // v = mix - inst
struct PitchVocoder {                                                                       // librosa.phase_vocoder, fp64 phase
    const float2* D;          // [signals][bins][T]
    float2* out;              // [signals][bins][Tout], Tout = ceil(T / rate)
    int bins, T, Tout, hop;
    double rate;
};
// the four lengths of one shift (vr_pitch_plan; csrc/pitch.hip): STFT frames, stretched frames, stretched samples, resampled samples
struct PitchPlan { int T, T_stretch; long long n_stretch, n_resampled; };
PitchPlan pitch_plan(long long L, int n_fft, int hop, double rate, double ratio);
void launch_pitch_diff(const float* mix, const float* inst, float* v, long long n, hipStream_t st);
void launch_phase_vocoder(const float2* D, float2* out, int signals, int bins, int T, int Tout, int hop, double rate, hipStream_t st);
// ---- plain training pairs (prepare.hip; vr_align_pair_many / vr_pair_rows_many) -----------------------------------
// Layout-compatible with vr_pair_window (include/vr_mi355.h): the trimmed ranges of the two waves, the lag of the mixture's head behind
// the instrumental's, and the common window -- n samples from a_off of the mixture and from b_off of the instrumental.
struct PairWindow { long long a_start, a_end, b_start, b_end, lag, a_off, b_off, n; };
// THE statement of the window arithmetic (vr_pair_window_plan; spec_utils.align_wave_head_and_tail's slicing): fills a_off, b_off, n from
// the other five; false when the window is empty (n <= 0)
inline bool pair_window_plan(PairWindow& w) {
    w.a_off = w.a_start;
    w.b_off = w.b_start;
    if (w.lag > 0) w.a_off += w.lag;
    else w.b_off -= w.lag;
    const long long na = w.a_end - w.a_off, nb = w.b_end - w.b_off;
    w.n = na < nb ? na : nb;
    return w.n > 0;
}
constexpr int kTrimFrame = 2048, kTrimHop = 512;     // librosa.effects.trim's defaults, top_db 60 (audio.trim)
// what the device keeps of one wave between the launches of a call: the trimmed range, the head's length and its mean
struct PrepState { long long start, end, nh; float mean, ref; };
// one wave of a call (2 per pair: the mixture 2 i, the instrumental 2 i + 1); a grid dimension picks the entry
struct PrepWave {
    const float* w;           // [2][L]
    long long L;
    long long head_cap;       // 4 * sr: the head is the first min(head_cap, end - start) trimmed samples
    int frames;               // 1 + L / kTrimHop
    float* rms;               // [2][frames]
    float* head;              // [min(head_cap, L)]
    PrepState* st;
};
struct LagCand { float v; int k; };                   // a correlation and its index in the 'full' sequence
constexpr int kLagParts = 64;                         // workgroups (and partial candidates) per pair of the argmax's first launch
struct PrepPair {
    const PrepState *sa, *sb;  // the two waves' states
    const float *a, *b;        // their heads
    float* full;               // [na + nb - 1] at most: np.correlate(a, b, 'full')
    LagCand* part;             // [kLagParts]
    PairWindow* out;           // the pair's window: the five measured fields
    int solo;                  // the pair has no second wave (trim only): sb = sa, no correlation, lag 0
};
// The forms of xcorr_full_kernel<FORM> (prepare.hip), one launch each over the call's table unless noted:
struct PrepRms { const PrepWave* tab; };              // rms[c][f] of every trim frame: one wave per (frame, channel), the squares summed in double
struct PrepTrim { const PrepWave* tab; };             // ref, first and last signal frame -> start, end; the head's sum in double -> its mean
struct PrepHeads { const PrepWave* tab; };            // head[j] = (w[0][start + j] + w[1][start + j]) - mean
struct XcorrTile { PrepPair p; };                     // ONE pair per launch: a block of kLagTile lags per workgroup, both heads through LDS
struct LagPart { const PrepPair* tab; };              // first maximum of `full`, per workgroup
struct LagPick { const PrepPair* tab; };              // ... of the partials; writes the pair's window
constexpr int kLagR = 8, kLagTile = 64 * kLagR, kLagChunk = 1024;
void launch_prep_trim(const PrepWave* tab_dev, int n_waves, int max_frames, long long max_head, hipStream_t st);
void launch_xcorr_tile(const PrepPair& p, long long nf_max, hipStream_t st);
void launch_lag_argmax(const PrepPair* tab_dev, int n_pairs, hipStream_t st);
// The conv families behind launch_conv.  A *_pick says whether its family takes the launch and fills the plan (kernel, MT, TH, TW);
// conv_plan (conv_mfma.hip) alone calls them, in its order.  A *_launch_conv takes tiled args (conv_fill_tiling) and the plan.
bool thin16_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);  // conv_thin.hip: <= 16 couts on v_mfma_f32_16x16x4_f32
void thin16_launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
bool wino_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);    // conv_wino.hip: Winograd F(2x2,3x3), 3x3 stride 1
void wino_launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
bool dma_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);     // conv_dma.hip: direct implicit GEMM, plain inputs by LDS-DMA
void dma_launch_conv(const ConvArgs& a, const ConvShape& s, const ConvPlan& p, hipStream_t st);
bool ws_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);      // conv_ws.hip: inputs with pending arithmetic, >= 32 columns
void ws_launch_conv(const ConvArgs& a, const ConvShape& s, const ConvPlan& p, hipStream_t st);
bool s2d_fused_eligible(const ConvArgs& a);                       // conv_dma.hip: stride-2 data gradient, four parity classes in one launch
void launch_s2d_fused(const ConvArgs& a, hipStream_t st);
struct S2WDesc { const float* w; float* wc; int Cin, Cout, CoutPad, CinPad; };          // one stride-2 layer; max_elems = max over layers of 4 * Cout * 9 * CinPad
void launch_s2_class_weights(const S2WDesc* d_descs, int n, long long max_elems, hipStream_t st);
void launch_wino_weights(const float* w, float* u, int Cin, int CoutPad, hipStream_t st);   // U = G g G^T
struct WinoWDesc { const float* w; void* u; int Cin, CoutPad; };                              // one layer of a batched refresh
void launch_wino_weights_batched(const WinoWDesc* d_descs, int n, long long max_elems, bool split6, hipStream_t st);
size_t wino_weights6_bytes(int Cin, int CoutPad);                                           // U as three bf16 planes (mfma_mode 2)
void launch_wino_weights6(const float* w, void* u6, int Cin, int CoutPad, hipStream_t st);
// conv_x3.hip: direct 3x3 stride-1 conv, fp32 products from six bf16 products (mfma_mode 2)
struct X3WDesc { const float* w; void* o; int Cin, KK, CoutPad; };                            // one layer of a batched weight split
bool x3_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);
void x3_launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st);   // ConvArgs::bf16 == 3: x3h_launch_conv
size_t x3_weights_bytes(int Cin, int KK, int CoutPad);
void launch_x3_weights(const float* w, void* o, int Cin, int KK, int CoutPad, hipStream_t st);
void launch_x3_weights_batched(const X3WDesc* d_descs, int n, long long max_elems, hipStream_t st);
// conv_x3h.hip: the same convs with fp32-grade products from three fp16 products (mfma_mode 3); weights in the SAME buffers
// (x3_weights_bytes), format [chunk][tap][2][CoutPad][8] fp16 + per-cout scale tails
void x3h_launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
bool x3h_tail_ok(const ConvArgs& a, const ConvPlan& p);  // a launch of plan p (CK_X3) with ConvArgs::tail set: a kernel with that second stage exists
void x3h_trace_read(long long* host, int n);          // diagnostics: phase stamps of the TRACE build (VR_CONV_DBG bit 64)
void x3h_trace_clear();
void launch_x3h_weights(const float* w, void* o, int Cin, int KK, int CoutPad, hipStream_t st);
void launch_x3h_weights_batched(const X3WDesc* d_descs, int n, long long max_elems, int max_cout_pad, hipStream_t st);
// conv_x3d.hip (round 6): conv_x3h's arithmetic for the 16-column layers -- dilated 3x3 (ASPP), 3x3 dilation 1 (enc5.conv2), 1x1 (ASPP conv2);
// weights in x3h format (launch_x3h_weights with KK = 9 / 1); mfma_mode 3 only
bool x3d_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);
void x3d_launch_conv(const ConvArgs& a, const ConvShape& s, const ConvPlan& p, hipStream_t st);
bool x3d_aspp_eligible(const ConvArgs* c4, const ConvShape* s4);   // c4 / s4 in concat order: 1x1, dilation (4,2), (8,4), (12,6)
// The module's pooled branch in eval, f1 = act(BN(conv1x1(mean over H of x5))), as a fifth part of that launch (option "aspp_pool_fused")
struct X3dPoolArgs {
    const float* x;            // x5 [N][C8][H][16], plain; null: no pooled part
    long long xN, xC, xH;
    const float* w;            // the 1x1 layer's K-major weights [C8][CoutPad]
    const float* epi;          // its folded BatchNorm [Cout][2], or null: no affine and no activation
    float slope;
    float* out;                // f1 [N][Cout][16] dense
    int C8, H, Cout, CoutPad;
};
bool x3d_pool_eligible(const X3dPoolArgs& q, const ConvArgs* c4);  // the group launch of c4 can carry q
void x3d_launch_aspp(const ConvArgs* c4, hipStream_t st, const X3dPoolArgs* pool = nullptr);   // the four branch convs of an ASPP module in ONE launch
// conv_x3s.hip: conv_x3h's arithmetic for the 3x3 STRIDE-2 layers with >= 32 output columns (eval, one plain source), the stride taken in the
// loader; weights in x3h format (KK = 9); mfma_mode 3 only
bool x3s_pick(const ConvArgs& a, const ConvShape& s, ConvPlan* p);
void x3s_launch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
void launch_upsample2x(const Tensor& x, float* out, hipStream_t st);   // dense [N][C][2H][2W], activated

// ---- lstm.hip -----------------------------------------------------------------------------------
// gx: [N][2*4H][T] input projections (+bias) for both directions; whh: [2][4H][H];
// out: [N][2H][T] (forward hidden in channels [0,H), reverse in [H,2H)).
void launch_bilstm(const float* gx, const float* whh_f, const float* whh_r, float* out,
                   int N, int T, int H, hipStream_t st);

// training variants: `save` [N][2][T][5H] keeps (i, f, g, o, c) per step for the backward pass
void launch_bilstm_train(const float* gx, const float* whh_f, const float* whh_r, float* out, float* save,
                         int N, int T, int H, hipStream_t st);
// dh [N][2H][T] (gradient at the LSTM output) -> dgx [N][8H][T] (gradient at the input projections)
void launch_bilstm_bwd(const float* dh, const float* save, const float* whh_f, const float* whh_r, float* dgx,
                       int N, int T, int H, hipStream_t st);
// dW_hh[dir][g][k] = sum_{n,t} dgx[n][dir*4H+g][t] * h_prev[n][dir*H+k][t]
size_t lstm_whh_grad_scratch_floats(int N, int H);      // floats of `part` below (one slab per sample slice and direction)
void launch_lstm_whh_grad(const float* dgx, const float* hout, float* dwhh_f, float* dwhh_r, int N, int T, int H,
                          int accumulate, float* part, hipStream_t st);

// ---- rows_gemm.hip ------------------------------------------------------------------------------
// out[n][co][t] = act((sum_k w[k][co] x[n][k][t] + bias[co]) * epi[co][0] + epi[co][1]): the LSTM input projection and the Linear behind
// the LSTM in eval, on v_mfma_f32_16x16x4_f32
struct RowsGemmArgs {
    const float* x;            // [N][K][T], samples xN floats apart
    long long xN;
    const float* w;            // [K][CoutPad] (a 1x1 conv's K-major weights)
    const float* bias;         // [Cout] or null
    const float* epi;          // folded BatchNorm [Cout][2] (scale, shift), or null: no affine and no activation
    float slope;               // activation slope behind the affine
    float* out;                // [N][Cout][T] dense
    int N, T, K, Cout, CoutPad;
};
bool rows_gemm_ok(const RowsGemmArgs& a);                        // the kernel takes this shape
int rows_gemm_tile(const RowsGemmArgs& a);                       // 22 / 21 / 11: (16 MC) couts x (16 NP) positions per workgroup, as MC NP
void launch_rows_gemm(const RowsGemmArgs& a, hipStream_t st, int tile = 0);   // tile 0: rows_gemm_tile's; the values do not depend on it

// ---- backward.hip -------------------------------------------------------------------------------
struct BnBwdArgs {
    float* g;                       // in: G (grad wrt post-activation value); out: dz (in place)
    const float* z;                 // raw conv output, same strides as g
    int N, C, H, W;
    long long sN, sC, sH;
    const float* aff;               // [C][2] scale, shift used in the forward (null = identity)
    int aff_bcast;                  // 1: C == 1 and the table is a broadcast copy (use row 0)
    float slope;
    const float* post;              // [N][C] dropout keep-mask or null
    const float *gamma, *save_mean, *save_invstd;
    float *dgamma, *dbeta;          // gradient arena slots
    int acc_grads;
    float* coef;                    // [C][3] scratch (kA, kB, kC); null = no BatchNorm (dz = dy)
    float* part;                    // [chunks][C][2] scratch
};
int bn_bwd_chunks(const BnBwdArgs& a);
void launch_bn_bwd(const BnBwdArgs& a, hipStream_t st);

void launch_upsample_bwd(const float* dhi, int N, int C, int H, int W, float* glo, long long gN, long long gC,
                         long long gH, int accumulate, hipStream_t st);
void launch_sum_h(const float* d, int N, int C, int H, int W, float* out, hipStream_t st);
void launch_avgpool_bwd(const float* gp, float* g, int N, int C, int H, int W, long long sN, long long sC, long long sH,
                        int accumulate, hipStream_t st);
void launch_thin_dgrad(const Tensor& x, int CO, const float* w, const float* dz, float* g, int accumulate, hipStream_t st);
int thin_wgrad_blocks(const Tensor& x);
void launch_thin_wgrad(const Tensor& x, int CO, const float* dz, float* part, float* dw, int accumulate, hipStream_t st);
void launch_reduce_rows(const float* part, long long stride, int P, float* out, long long n, int accumulate, float scale,
                        hipStream_t st);
int head_loss_blocks(const Tensor& x);
void launch_head_loss(const Tensor& x, const float* w, const float* X, const float* Y, int bins, float gscale,
                      float* dlogit, float* mask_out, float* loss_part, float* loss_out, float loss_scale, hipStream_t st);
void launch_head_bwd(const float* dmask, const float* mask, int N, int H, int W, int bins, float* dlogit, hipStream_t st);
// the complex-mask head (w [4][C]): X, Y, mask_out, dmask complex64 [N][2][bins][W], dlogit [N][4][H][W] (re ch0, re ch1, im ch0, im ch1);
// loss = sum |m X - y| over complex elements times loss_scale; head_bwd forms the logits again from x
void launch_head_loss_complex(const Tensor& x, const float* w, const float* X, const float* Y, int bins, float gscale,
                              float* dlogit, float* mask_out, float* loss_part, float* loss_out, float loss_scale, hipStream_t st);
void launch_head_bwd_complex(const Tensor& x, const float* w, const float* dmask, int bins, float* dlogit, hipStream_t st);
// The magnitude form of the complex head (VR_LOSS_MAG_L1_WAVE_SDR): the mask (always written) and
// loss_out[0] = loss_scale * sum | |y| - |m X| |; no dlogit -- the gradient of that loss needs batch-wide sums (launch_stft_wave_grad)
struct MagL1 {};                                      // the template tag of the magnitude forms (head_loss_kernel, l1_crop_kernel)
void launch_head_mag_l1(const Tensor& x, const float* w, const float* X, const float* Y, int bins, float* mask_out, float* loss_part,
                        float* loss_out, float loss_scale, hipStream_t st);
struct FlipDesc { const float* w; float* wt; int Cin, Cout, KK, CinPad, CoutPad; };
void launch_flip_transpose(const FlipDesc* d_descs, int n, hipStream_t st);
void launch_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double b1, double b2, double eps,
                 long long step, double gscale, hipStream_t st);
void launch_channel_sum(const float* d, int N, int C, int W, float* out, int accumulate, hipStream_t st);
void launch_f32_to_bf16(const float* x, unsigned short* y, long long n, hipStream_t st);
void launch_bf16_to_f32(const unsigned short* x, float* y, long long n, hipStream_t st);

// ---- model.hip (the product and the loss behind predict / validate_step) -------------------------
// m [rows][Wm] *= x [rows][T] at columns off .. off + Wm; cplx: both complex64, the complex product
void launch_mul_crop(const float* x, float* m, bool cplx, long long rows, int T, int Wm, int off, hipStream_t st);
// loss[0] = mean |pred [rows][Wm] - y [rows][T] at columns off .. off + Wm|; part: scratch of l1_crop_blocks() floats
// form L1_CROP_COMPLEX: complex64 pred and y, mean |pred - y| over complex elements (rows and columns count complex elements);
// L1_CROP_MAG: the same on their magnitudes, mean | |pred| - |y| |
int l1_crop_blocks();
enum L1CropForm { L1_CROP_REAL = 0, L1_CROP_COMPLEX = 1, L1_CROP_MAG = 2 };
void launch_l1_crop(L1CropForm form, const float* pred, const float* y, long long rows, int T, int Wm, int off, float* part, float* loss,
                    hipStream_t st);

// ---- stft.hip -----------------------------------------------------------------------------------
struct FFTPlan { int n_fft; int log2n; float2* twiddle; float* window; };
// wave [2][L] -> spec [2][bins][T] complex64
void launch_stft(const FFTPlan& pl, const float* wave, long long L, int hop, int T, float2* spec, hipStream_t st);
// spec [2][bins][T] -> frames scratch [2][T][n_fft] -> wave [2][hop*(T-1)]
void launch_istft(const FFTPlan& pl, const float2* spec, int hop, int T, float* frames, float* wave, hipStream_t st);
// The per-frame kernels on any number of signals in one grid, whatever the hop (the pitch shifter's transforms):
// wave [signals][L] -> spec [signals][bins][T];  spec [signals][bins][T] -> frames scratch [signals][T][n_fft] -> wave [signals][length],
// length samples of the overlap-add behind the n_fft / 2 in front (librosa.istft(length=)): cut, or zeros past the last frame
void launch_stft_signals(const FFTPlan& pl, const float* wave, long long L, int hop, int T, int signals, float2* spec, hipStream_t st);
void launch_istft_length(const FFTPlan& pl, const float2* spec, int hop, int T, int signals, float* frames, float* wave, long long length,
                         hipStream_t st);
// the rows form of the frame-tiled STFT (hop == n_fft / 2): wave [2][L] -> rows [T][2][bins], the training cache's layout, the values
// launch_stft's
struct SpecRows {};
void launch_stft_rows(const FFTPlan& pl, const float* wave, long long L, int T, float2* rows, hipStream_t st);
// Fused form for hop == n_fft/2: wave = istft(m * spec) (which 0) or istft(spec - m * spec) (which 1); mask_a null = plain
// istft.  No frame buffer, no materialised y / v spectrograms (inference.py:26-40 + lib/spec_utils.py:157-165 in one pass).
bool istft_masked_available(const FFTPlan& pl, int hop);
void launch_istft_masked(const FFTPlan& pl, const float2* spec, int hop, int T, const float* mask_a, int Wa, const float* mask_b,
                         int Wb, int shift, const float* wgt, int which, float* wave, hipStream_t st);
// The sample-format forms of the two tile kernels (hop == n_fft / 2 only; csrc/pcm.h): the STFT reads interleaved WAV sample bytes, the
// masked iSTFT (mask_a null: plain) writes interleaved int16 [hop * (T-1)][2] = pcm16_from_float of the float it would have stored.
struct PcmIn { const uint8_t* bytes; int channels; int fmt; };   // frames of `channels` (1: up-mixed) samples, fmt = vr_pcm_format
void launch_stft_pcm(const FFTPlan& pl, const PcmIn& in, long long L, int T, float2* spec, hipStream_t st);
// the crop-table form of the frame-tiled STFT (the wave store of vr_dataset_*): one entry per signal, grid (frame
// tile, channel, entry).  Entry e writes rows [start, start + T) of the STFT of its wave -- n samples per channel, the zero padding at the
// wave's own ends -- to dst as [T][2][bins] complex64, the values launch_stft_rows gives for the whole wave.  fmt 0: `wave` is planar
// float32 [2][n]; otherwise interleaved frames of `channels` (1: up-mixed) samples in that vr_pcm_format, read through WavePcmIn.  The
// host keeps 0 <= start and start + T <= 1 + n / hop: the kernel checks samples against n, never rows against the song.
struct CropSeg { const void* wave; long long n; long long start; float2* dst; int T; int fmt; int channels; int reserved; };
bool stft_crops_supported(int n_fft, int hop);           // no device: the frame-tiled path takes this n_fft at hop == n_fft / 2
void launch_stft_crops(const FFTPlan& pl, const CropSeg* table_dev, int entries, int max_T, double rows_total, hipStream_t st);
void launch_istft_masked_pcm16(const FFTPlan& pl, const float2* spec, int hop, int T, bool cplx, const float* mask_a, int Wa,
                               const float* mask_b, int Wb, int shift, const float* wgt, int which, int16_t* out, hipStream_t st);
// mag_pad [2][bins][Wpad] (pre-zeroed) <- |spec| at column pad_l + t; maxima into stats:
// per-row partial maxima into stats (16 B header + 2 x bins rows of (max |X| bits, 64-bit lexicographic complex key))
void launch_mag_pad(const float2* spec, int bins, int T, float* mag_pad, int Wpad, int pad_l,
                    unsigned* stats, hipStream_t st);
// aff[0..3] = (1/coef, 0, 1/coef, 0), coef = max|X| (mode 0) or |lexicographic max| (mode 1)
void launch_coef_affine(unsigned* stats, int rows, int mode, float* aff, hipStream_t st);   // rows = 2 * bins partials
// complex handle: 1/c as a complex number, c = max|X| (mode 0) or the lexicographic complex max itself (mode 1)
void launch_coef_complex(unsigned* stats, int rows, int mode, float2* inv, hipStream_t st);
// spec [N][2][bins][T] complex64 -> dst [N][4][bins][Wdst] planar (re ch0, re ch1, im ch0, im ch1), frame t at column pad_l + t,
// every other column zero; times *scale (complex, may be null)
void launch_pack_complex(const float2* spec, int N, int bins, int T, float* dst, int Wdst, int pad_l, const float2* scale,
                         hipStream_t st);
// y = m*X, v = (1-m)*X with m = mask_a[.., t] (tta=0) or 0.5*(mask_a[.., t] + mask_b[.., t + shift])
// wgt [T] (or null): per-frame merge_artifacts weight, m += wgt[t] * (1 - m)
void launch_apply_mask(const float2* spec, int bins, int T, const float* mask_a, int Wa,
                       const float* mask_b, int Wb, int shift, const float* wgt, float2* y, float2* v, hipStream_t st);
// fmin[t] = min over (channel, bin) of the final mask at frame t
void launch_frame_min(int bins, int T, const float* mask_a, int Wa, const float* mask_b, int Wb, int shift, float* fmin,
                      hipStream_t st);
// the same three for a complex64 mask: complex products; the TTA average is complex; merge_artifacts blends |m| and keeps the
// phase, m' = (|m| + wgt (1 - |m|)) m / |m| (m = 0: m' = wgt); the frame minimum is taken over |m|
void launch_apply_mask_complex(const float2* spec, int bins, int T, const float2* mask_a, int Wa, const float2* mask_b, int Wb,
                               int shift, const float* wgt, float2* y, float2* v, hipStream_t st);
void launch_istft_masked_complex(const FFTPlan& pl, const float2* spec, int hop, int T, const float2* mask_a, int Wa,
                                 const float2* mask_b, int Wb, int shift, const float* wgt, int which, float* wave, hipStream_t st);
void launch_frame_min_complex(int bins, int T, const float2* mask_a, int Wa, const float2* mask_b, int Wb, int shift, float* fmin,
                              hipStream_t st);

// ---- the wave-domain SDR term of a complex train / validate step (VR_LOSS_MAG_L1_WAVE_SDR; hop == n_fft / 2) --
// The pair form of istft_tile_kernel takes this as its source (one entry in device memory): `signals` spectrograms [bins][T] each of the
// target y and of the estimate p = mask * x (mask null: x is the estimate itself).  One workgroup runs the same frame tile of y and
// of p, stores both waves [signals][hop (T-1)] and leaves its partial sums (<y, p>, <y, y>, <p, p>) in part [signals * blocks][3].
struct WavePair {
    const float2* x;          // [signals][bins][x_pitch]
    const float2* mask;       // [signals][bins][x_pitch] or null
    const float2* y;          // [signals][bins][y_pitch], frame t at column y_off + t
    int x_pitch, y_pitch, y_off;
    float* y_wave;            // [signals][hop (T-1)]
    float* p_wave;
    float* part;              // [signals * wave_pair_blocks()][3]
};
bool wave_loss_available(const FFTPlan& pl, int hop);        // the tile kernels take this n_fft and hop
int wave_pair_blocks(const FFTPlan& pl, int T);              // workgroups per signal (0: T < 2, no samples)
void launch_istft_pair(const FFTPlan& pl, const WavePair* pair_dev, const WavePair& pair, int signals, int T, hipStream_t st);
// The adjoint: the gradient form of stft_tile_kernel.  Its wave source is (alpha y_wave + beta p_wave) / envelope with alpha, beta from
// the three sums in device memory (d sdr / d p_wave = -y_wave / D + (a p / (q D^2)) p_wave, times sdr_scale); its store epilogue scales
// by c_k / n_fft, zeroes the imaginary parts of DC and Nyquist, adds the magnitude-L1 gradient l1_scale sgn(|p| - |y|) p / |p|
// (l1_scale 0: off, mask and Y are not read) and multiplies by conj(X): dmask [signals][bins][T] complex64, dL/dRe + i dL/dIm.
struct WaveGrad {
    const float* y_wave;      // [signals][hop (T-1)]
    const float* p_wave;
    const float* sums;        // [3]: <y, p>, <y, y>, <p, p>
    const float2* X;          // [signals][bins][T]
    const float2* mask;
    const float2* Y;
    float2* dmask;
    float sdr_scale;          // sdr_weight / accumulation_steps
    float l1_scale;           // 1 / (n_el accumulation_steps)
};
void launch_stft_wave_grad(const FFTPlan& pl, const WaveGrad& g, int signals, int T, hipStream_t st);

// ---- the weighted SDR term (VR_LOSS_MAG_L1_WAVE_WSDR; the reference's weighted_sdr_loss, train.py:53-65) -------
// The triple form of istft_tile_kernel: one workgroup runs the same frame tile three times -- the mixture x, the target y, the estimate
// p (mask * x, the product fused into the tile load; mask null: the materialised `p`) -- stores the three waves [signals][hop (T-1)] and
// leaves its six partial sums in part [signals * wave_pair_blocks()][6], in this order, with n = x_wave - y_wave and q = x_wave - p_wave
// formed sample by sample:  <y, p>, <y, y>, <p, p>, <n, q>, <n, n>, <q, q>.
struct WaveTriple {
    const float2* x;          // [signals][bins][xy_pitch], frame t at column xy_off + t
    const float2* y;          // the same layout
    const float2* mask;       // the same layout, or null
    const float2* p;          // (mask null) [signals][bins][p_pitch], frame t at column t
    int xy_pitch, xy_off, p_pitch;
    float* x_wave;            // [signals][hop (T-1)]
    float* y_wave;
    float* p_wave;
    float* part;              // [signals * wave_pair_blocks()][6]
};
void launch_istft_triple(const FFTPlan& pl, const WaveTriple* triple_dev, const WaveTriple& triple, int signals, int T, hipStream_t st);
// The three coefficients of d wsdr / d p_wave = cy y_wave + cp p_wave + cx x_wave from the six sums, in double;
// a term whose estimate norm is 0 is 0 (torch's linalg.norm backward at a zero vector).  Host and device.
struct WsdrCoef { double cy, cp, cx; };
__host__ __device__ inline WsdrCoef wsdr_coefficients(double A1, double yy, double pp, double A2, double nn, double qq) {
    const double eps = 1e-8;
    const double P1 = sqrt(yy), Q1 = sqrt(pp), P2 = sqrt(nn), Q2 = sqrt(qq), D1 = P1 * Q1 + eps, D2 = P2 * Q2 + eps;
    const double alpha = yy / (yy + nn + eps);
    const double k1 = Q1 > 0.0 ? alpha * A1 * P1 / (Q1 * D1 * D1) : 0.0;
    const double k2 = Q2 > 0.0 ? (1.0 - alpha) * A2 * P2 / (Q2 * D2 * D2) : 0.0;
    return WsdrCoef{-alpha / D1 - (1.0 - alpha) / D2, k1 + k2, (1.0 - alpha) / D2 - k2};
}
// The three-wave gradient form of stft_tile_kernel: WaveGrad with the wave source (cy y_wave + cp p_wave + cx x_wave) sdr_scale / envelope,
// the coefficients formed on the device from the six sums; the store epilogue is WaveGrad's.
struct WaveGrad3 {
    const float* x_wave;      // [signals][hop (T-1)]
    const float* y_wave;
    const float* p_wave;
    const float* sums;        // [6], WaveTriple's order
    const float2* X;          // [signals][bins][T]
    const float2* mask;
    const float2* Y;
    float2* dmask;
    float sdr_scale;          // sdr_weight / accumulation_steps
    float l1_scale;           // 1 / (n_el accumulation_steps)
};
void launch_stft_wave_grad3(const FFTPlan& pl, const WaveGrad3& g, int signals, int T, hipStream_t st);

// ---- the wave term of either kind, as every caller runs it (validate step, train-form head, the wave_pair / wave_triple hooks) --------
// The caller states sources, pitches, offset, waves and partials in the kernel's own table entry (WavePair: kind 1, WaveTriple: kind 3).
// launch_wave_term copies the entry to table_dev (64 floats) -- through `staging`, which must outlive the copy, on the stream; staging
// null: synchronously -- launches the pair or triple form of istft_tile_kernel over `signals` spectrograms of T >= 2 frames and sums the
// partials into sums [3] or [6].
union WaveTable { WavePair pair; WaveTriple triple; };
void launch_wave_term(const FFTPlan& pl, const WavePair& pair, float* table_dev, WaveTable* staging, int signals, int T, float* sums,
                      hipStream_t st);
void launch_wave_term(const FFTPlan& pl, const WaveTriple& triple, float* table_dev, WaveTable* staging, int signals, int T, float* sums,
                      hipStream_t st);
// what a wave term of loss kind 1 / 3 needs, in floats: `waves` waves of `wave` each, the partial sums, the table entry's slot
struct WaveTermFloats { int waves; size_t wave, part, table; };
WaveTermFloats wave_term_floats(const FFTPlan& pl, int hop, int kind, int signals, int T);

// ---- many songs in one call (vr_separate_many / vr_separate_wave_many) ----------------------------------------------------------
// One entry of the call's song table (built on the host, one copy to the device).  The crops of all songs, and of both TTA passes, form
// ONE crop list (pass-major, song-major inside a pass): crop n's mask lands at column n * roi of one concatenated mask
// [2][bins][W] (complex64 for a complex handle), so a device batch may hold crops of several songs and of both passes.
struct SongSeg {
    const float* wave;        // [2][L]           (wave-level calls)
    long long L;
    float2* spec;             // [2][bins][T]     (read; written by the STFT of a wave-level call)
    float2* y;                // [2][bins][T]     instruments, vocals (spectrogram-level calls)
    float2* v;
    float* y_wave;            // [2][hop * (T-1)] (wave-level calls)
    float* v_wave;
    int T;
    int mcol_a, mcol_b;       // column of the song's frame 0 in the concatenated mask: pass 0, TTA pass 1
    int frame0;               // the song's first slot in the call's per-frame merge_artifacts weights
    float* fmin;              // [T] the song's per-frame mask minima (--postprocess)
};
bool many_tiled_available(const FFTPlan& pl, int hop);       // hop == n_fft / 2: the tile kernels below exist
// pcm (device, one per song): the songs' sample bytes are read in place of the table's `wave` (pcm_bytes: the profiler's note)
void launch_stft_many(const FFTPlan& pl, const SongSeg* songs, int n_songs, int max_T, double sum_L, double sum_T, hipStream_t st,
                      const PcmIn* pcm = nullptr, double pcm_bytes = 0.0);
// part [song][2 * bins][2]: per-row partial maxima (max |X| bits, lexicographic complex key); aff [song][4]: 1 / c as launch_coef_affine
// (cplx: launch_coef_complex) gives it
void launch_song_stats(const SongSeg* songs, int n_songs, int bins, double sum_T, unsigned long long* part, hipStream_t st);
void launch_song_coef(const unsigned long long* part, int n_songs, int rows, int mode, bool cplx, float* aff, hipStream_t st);
// crops[n] = (song, first frame; may be negative): dst [count][nin][max_bin][cropsize] = the normalised network input, zero outside the song
void launch_crop_gather(const SongSeg* songs, const int2* crops, int count, bool cplx, int bins, int max_bin, int cropsize, const float* aff,
                        float* dst, hipStream_t st);
void launch_frame_min_many(const SongSeg* songs, int n_songs, int max_T, int bins, const float* mask, int W, int tta, bool cplx,
                           hipStream_t st);
void launch_apply_mask_many(const SongSeg* songs, int n_songs, int max_T, int bins, const float* mask, int W, int tta, bool cplx,
                            const float* wgt, hipStream_t st);
void launch_istft_masked_many(const FFTPlan& pl, const SongSeg* songs, int n_songs, int max_T, double sum_T, const float* mask, int W, int tta,
                              bool cplx, const float* wgt, int which, hipStream_t st, bool pcm16 = false);   // pcm16: y_wave / v_wave are int16 [samples][2]

// ---- evaluation against the true stems (vr_evaluate_wave*; hop == n_fft / 2) -------------------------------------
// One entry per song beside the song table (device memory): the evaluation form of istft_tile_kernel takes the table entry's mixture
// (`wave`, `L`) and this song's true instruments, and leaves per segment of hop samples the double sums of the reference squares and of the
// error squares of the segment's lower and upper window (window >= hop: at most two).  `which` 0 measures the instruments against
// inst, 1 the vocals against mix - inst.  The estimate is the float the plain form stores; `store` 0: it is not stored at all (y_wave /
// v_wave of the table may then be null).
struct WaveEval {
    const float* inst;        // [2][L], L of the table entry
    double* part;             // [stem 2][channel 2][segment T-1][wave 4][4] = (reference lower, error lower, reference upper, error upper)
    double* sums;             // [n_windows][4] = sum r_y^2, sum (r_y - y)^2, sum r_v^2, sum (r_v - v)^2   (launch_eval_sums)
    long long window;         // samples per window, >= hop
    int store;
};
size_t eval_part_doubles(int T);                             // doubles of `part` for a song of T frames
int eval_tile_step(const FFTPlan& pl);                       // segments per workgroup of the tile kernel (the hook reports it)
// mask_a / mask_b / shift as istft_tile_kernel documents them for the song table (the executor: mask_b = mask_a or null, Wb = Wa, shift 0);
// stored: whether any entry stores its stems (the profiler's note)
void launch_istft_eval_many(const FFTPlan& pl, const SongSeg* songs, const WaveEval* evs, int n_songs, int max_T, double sum_T, const float* mask_a,
                            int Wa, const float* mask_b, int Wb, int shift, bool cplx, const float* wgt, int which, bool stored, hipStream_t st);
// sums[w][q] of every song = its partials of window w added over (segment, channel, wave) in a fixed order; max_windows: the largest count
void launch_eval_sums(const FFTPlan& pl, const SongSeg* songs, const WaveEval* evs, int n_songs, long long max_windows, double sum_T, hipStream_t st);

// ---- pseudo-instrument labels (vr_pseudo*) ------------------------------------------------------------------------
// One entry per song beside the song table (device memory), as WaveEval rides beside it: the plain table forms keep their entry and
// their code.  The pair takes the place of the one input: the table's `spec` is D = X - Y (what the network separates), written by the
// pair front end; the back end stores P = Y + instruments stem of D and nothing else.
struct PseudoSeg {
    const float* inst_wave;   // [2][L] the imperfect instrumental, L of the table entry (wave-level calls)
    const float2* mix;        // [2][bins][T] X (spectrogram-level calls; a wave-level call never writes X)
    float2* inst;             // [2][bins][T] Y (read; written by the pair STFT of a wave-level call)
    float2* out;              // P: [2][bins][T] (VR_PSEUDO_SPEC) or [T][2][bins] (VR_PSEUDO_ROWS)
};
// the pair form of stft_tile_kernel: mixture tile and instrumental tile of the same frames in one workgroup; stores Y and D = X - Y
void launch_stft_pseudo_many(const FFTPlan& pl, const SongSeg* songs, const PseudoSeg* ps, int n_songs, int max_T, double sum_L, double sum_T,
                             hipStream_t st);
// D = X - Y over the song table, one workgroup per (row, song)
void launch_pseudo_diff_many(const SongSeg* songs, const PseudoSeg* ps, int n_songs, int bins, double sum_T, hipStream_t st);
// the pseudo form of apply_mask_kernel: out = Y + instruments stem; rows: out is [T][2][bins], written through an LDS tile
void launch_apply_mask_pseudo_many(const SongSeg* songs, const PseudoSeg* ps, int n_songs, int max_T, int bins, const float* mask, int W, int tta,
                                   bool cplx, const float* wgt, bool rows, double sum_T, hipStream_t st);

// ---- spectrogram images (vr_spec_image*, vr_separate_*_img) ---------------------------------------------------------
// One entry per image job of a call (device memory).  A job is one min / max range and the pictures scaled by it: a stored spectrogram
// gives one picture (img[0]); a song of a separation call gives two, instruments and vocals, each with a range of its own, and rides
// beside the song table as PseudoSeg does.  A picture of a two-channel source is [bins][T][3] bytes (max(L, R), L, R), of a one-channel
// source [bins][T].  The range pass leaves per workgroup (min y, max y) of either stem in part[workgroup]; the write pass reduces them
// again in every workgroup and leaves (lo, max - lo) per stem in `range`.
constexpr int kImgChunk = 1024;       // pixels per workgroup step of either pass
constexpr int kImgParts = 512;        // most workgroups of a job's range pass
constexpr int kImgWriteChunks = 4;    // chunks per workgroup of the write pass
struct ImgSeg {
    const void* src;          // [channels][bins][T] complex64 or float32 (stored spectrograms; unused beside a song table)
    uint8_t* img[2];
    float4* part;             // [kImgParts] (min, max) of stem 0, (min, max) of stem 1
    float* range;             // [stems][2]
    int T;
};
// n stored spectrograms: one range launch and one write launch for all of them; max_T, sum_T: the longest job, all jobs (profiler's note)
void launch_spec_image_many(const ImgSeg* jobs, int n, int channels, int bins, int max_T, double sum_T, bool cplx, int mode, hipStream_t st);
// the two stems of every song of a separation call, from the song's spectrogram and the call's mask as apply_mask_kernel reads them
void launch_stem_image_many(const SongSeg* songs, const ImgSeg* jobs, int n_songs, int max_T, int bins, const float* mask, int W, int tta, bool cplx,
                            const float* wgt, double sum_T, hipStream_t st);
// vr_spec_image_many behind its argument checks: staging, the two launches, the copies back
void spec_image_many_api(int device, int n, const void* const* specs, bool on_dev, int channels, int bins, const int* T, bool cplx, int mode,
                         uint8_t* const* imgs, bool out_on_dev, float* ranges);

// ---- streaming separation (vr_stream_*) ------------------------------------------------------------------------------------------
// The state of one step of a stream, as the StreamSeg instantiations of the spectrogram-side kernels read it (one copy to the device per
// step).  The kernels take a TABLE of them: one grid dimension is the table entry, sized for the largest entry, and a workgroup past
// its own entry's frame or segment count leaves at once.  One executor fills and launches the table, Model::stream_run: vr_stream_push
// gives it one entry, vr_stream_push_many one per stream of a round; the statistics pass alone reads a single entry (seg + e).
// Samples and frames carry their ABSOLUTE index in the stream; the device keeps rings: frame t of the complex spectrogram at
// column t % R of ring [2][bins][R], the mask of frame t at column t % RM of mask_a [2][bins][RM] (complex64 for a complex handle) and,
// for the TTA pass, at column (t + shift) % RM of mask_b (the offline layout: crop j of a pass at column j * roi).
struct StreamSeg {
    // samples: p < blk_base lives in tail[ch * tail_pitch + p - tail_base], p >= blk_base in blk[ch * blk_pitch + p - blk_base];
    // outside [0, L) a sample is zero (centre padding in front; behind the data only the flush step's last frame reaches there)
    const float* tail;
    const float* blk;
    float* tail_out;          // the STFT step leaves the samples [tail_out_base, L) here for the next step (never the buffer it reads)
    long long tail_base, blk_base, blk_pitch, tail_out_base;
    long long L;              // samples received so far, this step's block included
    int tail_pitch;
    // frames
    float2* ring;
    int R;
    int t_new;                // the STFT writes the frames [t_new, T); the statistics pass reads the same ones
    int T;                    // frames valid so far; the true frame count once flushed (the crop gather writes zero outside [0, T))
    // masks
    const float* mask_a;
    const float* mask_b;      // null without TTA
    int RM, shift;
    const float* aff;         // 1 / c of this stream as the crop gather reads it (launch_coef_affine / launch_coef_complex)
    // masked iSTFT of the frames [t_out, t_done): segment s = second half of frame s + first half of frame s + 1 lands at
    // wave[ch * out_pitch + (s - t_out) * hop]; `carried`: frame t_out was transformed by the previous step, its windowed second half
    // comes from carry_in; the second half of frame t_done - 1 goes to carry_out ([stem][ch][hop], never the buffer read)
    int t_out, t_done, carried;
    const float* carry_in;
    float* carry_out;
    float* y_wave;
    float* v_wave;
    long long out_pitch;
    // --postprocess (fmin_ring null: not a postprocess stream, and the masked iSTFT blends nothing): the minima of the
    // frames [fm_lo, fm_hi), whose masks became final in this step, go to fmin_ring[t % RW]; the walk (stream_post.h) takes them from
    // there, moves `post` on and writes the merge_artifacts weight of frame t at wgt_ring[t % RW]; post_flush: the stream ends with frame
    // fm_hi - 1.  The masked iSTFT reads wgt_ring for its frames, which lie kStreamPostDelay below fm_hi (or, flushed, anywhere below it).
    float* fmin_ring;
    float* wgt_ring;
    StreamPostState* post;
    int RW, fm_lo, fm_hi, post_flush;
};
bool stream_tiled_available(const FFTPlan& pl, int hop);
// seg: a device table of n_seg entries; new_frames = the largest count of new frames among them, new_samples / sum_* only size the profiler's note
// pcm (device, one per entry): the blocks of this round are sample bytes, read in place of the entries' `blk` from the block's first frame on
// (pcm_bytes: the profiler's note)
void launch_stft_stream(const FFTPlan& pl, const StreamSeg* seg, int n_seg, int new_frames, double new_samples, double sum_frames, hipStream_t st,
                        const PcmIn* pcm = nullptr, double pcm_bytes = 0.0);
// part: per-row partial maxima as launch_mag_pad leaves them (stats + 16 bytes); the new frames are reduced INTO them
void launch_stream_stats(const StreamSeg* seg, int bins, int new_frames, unsigned long long* part, hipStream_t st);
// crops[n] = (table entry, first frame; may be negative): as launch_crop_gather, from the entry's ring, times the entry's 1 / c
void launch_stream_gather(const StreamSeg* seg, const int2* crops, int count, bool cplx, int bins, int max_bin, int cropsize, float* dst,
                          hipStream_t st);
// segments = the largest count of output segments among the n_seg entries (an entry with none is skipped); sum_segments, tta: profiler's note
void launch_istft_stream(const FFTPlan& pl, const StreamSeg* seg, int n_seg, int segments, double sum_segments, bool cplx, bool tta, int which,
                         hipStream_t st, bool pcm16 = false);         // pcm16: y_wave / v_wave are int16 [capacity][2]
// the postprocess entries of the table (the others are skipped): the minima of their frames [fm_lo, fm_hi) -- post_frames = the largest
// count among them, sum_frames: profiler's note; no launch when 0 -- then the walk, one workgroup per entry (walk false: no entry has
// new minima or a flush).  Both are forms of frame_min_kernel.
void launch_stream_post(const StreamSeg* seg, int n_seg, int post_frames, double sum_frames, bool walk, bool cplx, bool tta, int bins,
                        hipStream_t st);

}  // namespace vr
