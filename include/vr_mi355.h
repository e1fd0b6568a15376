/* libvr_mi355.so -- C ABI of the MI355X-native vocal-remover hot path.
 *
 * The reference (tsurumeso/vocal-remover @ 2024_08_07) has no FFI layer: its boundary is the Python
 * API that inference.py / train.py / pseudo.py call.  Each entry point below names the reference
 * interface it replaces; vocal-remover_amd/ binds them with ctypes and re-exposes the reference's
 * class / function names.
 *
 * Conventions
 *   - every function returns 0 on success or a negative vr_status; the message of the last failure
 *     on the calling thread is vr_last_error().  Nothing aborts, nothing calls back into the host.
 *   - `*_on_device` flags say whether a data pointer is host memory (numpy / torch CPU,
 *     C-contiguous) or device memory on the handle's GPU.  The caller owns every pointer it passes;
 *     the library copies.  The library owns all device memory it allocates (weights, workspace).
 *   - a handle is bound to one GPU and one HIP stream and is not thread-safe; use one handle per
 *     process per GPU.  Calls return after the handle's stream has drained.
 *   - tensors are fp32; spectrograms are complex64 stored as interleaved (re, im) floats with the
 *     reference's layout [2, n_fft/2+1, frames]; waves are [2, samples].
 */
#ifndef VR_MI355_H
#define VR_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vr_model* vr_handle;

enum vr_status {
    VR_OK = 0,
    VR_ERR_UNKNOWN = -1,
    VR_ERR_BAD_ARGUMENT = -2,   /* shape / key / flag errors                                      */
    VR_ERR_HIP = -3,            /* a HIP runtime call failed                                       */
    VR_ERR_OOM = -4,            /* workspace planning / allocation failure                         */
    VR_ERR_CROP_CENTER = -5,    /* reference ValueError of spec_utils.crop_center (spec_utils.py:15) */
    VR_ERR_EMPTY_MASK = -6,     /* reference `assert mask.size()[3] > 0` (nets.py:129,139)         */
    VR_ERR_INDEX = -7,          /* reference IndexError in merge_artifacts (spec_utils.py:65, empty idx) */
    VR_ERR_COMM = -8,           /* RCCL could not be loaded, or a collective failed                        */
    VR_ERR_UNSUPPORTED = -9     /* the handle has no kernel for this request (vr_pair_rows_many: hop_length != n_fft / 2); the caller's other route applies */
};

const char* vr_last_error(void);

/* nets.CascadedNet(n_fft, hop_length, nout=32, nout_lstm=128)        lib/nets.py:46-80
 * (is_complex=False, the only configuration any reference caller uses).                           */
int vr_create(int device, int n_fft, int hop_length, int nout, int nout_lstm, vr_handle* out);
/* The same with flags.  VR_CREATE_COMPLEX: nets.CascadedNet(..., is_complex=True) -- nin = 4 input channels
 * [re L, re R, im L, im R], so the first layers and out / aux_out take their nin = 4 shapes (vr_param_info), and a
 * complex mask bounded by tanh(|m|) (lib/nets.py:104-107,119-122).  By default such a handle runs eval-mode inference only
 * (training it is opt-in per handle: vr_set_option "complex_train" below):
 *   vr_forward      x and out are complex64 (interleaved re, im): x [B,2,bins,T], out [B,2,bins,Wm] in every mode;
 *                   in training mode it returns VR_ERR_BAD_ARGUMENT
 *   vr_separate / vr_separate_wave   same signatures; the network sees the complex crops (X_pad / c, with c = max|X|,
 *                   or for tta numpy's lexicographic complex maximum as a complex divisor), TTA averages the complex masks,
 *                   --postprocess blends |mask| and keeps its phase, y = mask X and v = (1 - mask) X are complex products
 *   vr_train_step, vr_forward_train, vr_backward, vr_validate_step   VR_ERR_BAD_ARGUMENT (training is not supported)
 *   vr_set_mode(h, 1) is accepted (model.train()).
 * With vr_set_option(h, "complex_train", 1) the same entry points train it (train.py:77-96 on complex tensors).  X, y, mask_out and
 * dmask are then complex64 [B,2,bins,T] (interleaved re, im), as vr_forward takes them:
 *   vr_train_step      loss = mean |mask X - y| over the B*2*bins*T complex elements (torch's L1Loss on complex tensors); the
 *                      gradient of |d| at d = 0 is 0, and so is that of the bound at a zero logit pair
 *   vr_forward_train / vr_backward   dmask in torch's convention for a real loss: dL/dRe(mask) + i dL/dIm(mask)
 *   vr_forward         in training mode: batch statistics and the running update, live Dropout2d, as on a magnitude handle
 *   vr_validate_step   eval mode only: mean |crop(X mask) - crop_center(y)| as a complex difference
 * Tested in the default "mfma_mode" with "train_winograd" 0 and 1; the other modes run.                  */
#define VR_CREATE_COMPLEX 1
int vr_create_ex(int device, int n_fft, int hop_length, int nout, int nout_lstm, int flags, vr_handle* out);
int vr_destroy(vr_handle h);

/* nn.Module.state_dict() / load_state_dict()                  inference.py:131, train.py:209,290
 * One call per state-dict key (689 keys for the default net), torch shapes and layouts
 * (conv OIHW, LSTM [4H, I], gate order i,f,g,o).  num_batches_tracked entries are int64.        */
int vr_num_params(vr_handle h);
int vr_param_info(vr_handle h, int index, char* key_buf, int key_cap, int64_t* shape4, int* ndim,
                  int* is_int64, int* trainable);
int vr_set_param(vr_handle h, const char* key, const void* host, const int64_t* shape, int ndim);
int vr_get_param(vr_handle h, const char* key, void* host, int64_t capacity_bytes);

/* nn.Module.train() / eval()                                          inference.py:52, train.py:69,109 */
int vr_set_mode(vr_handle h, int training);
/* Numerical options.  "train_winograd" (default 1): train-mode forward and data-gradient 3x3 stride-1
 * convolutions may use the transformed-weight kernels (mfma_mode 0: Winograd F(2x2,3x3), fp32, rounding differs from the direct
 * kernel by ~1e-6 relative per conv -- the same class of difference as cuDNN's algorithm choice in the reference; mfma_mode 3 / 2:
 * the split direct kernels conv_x3h.hip / conv_x3.hip); 0 = the fp32 direct kernels only.  Eval follows "mfma_mode" alone.
 * "adam_reset": zero the Adam moments and the step counter (what constructing a new
 * torch.optim.Adam does; train.py:215-218).  "serial_exec" (default 0): 1 = every kernel on the handle's one
 * stream, no lanes / side streams (tests: results must not depend on the concurrent executor).
 * "mfma_mode" (default 3): how the 3x3 stride-1 convolutions (84 % of the multiply-adds) form their products.
 *   3 = fp32-grade products from THREE fp16 products: every operand is scaled by an exact power of two (weights per output channel,
 *       pixels per workgroup tile and 8-channel chunk, the accumulators follow) and written as two fp16 numbers (22 significand
 *       bits), a*b ~= a1b1 + a1b2 + a2b1 with fp32 accumulation on v_mfma_f32_32x32x16_f16 -- conv_x3h.hip, forward and data
 *       gradient, 14 matrix instructions per 8-channel chunk; measured error against fp64 at or below mode 2's and an fp32 direct
 *       convolution's (tests), any fp32 dynamic range (2^+-100 scales, subnormals) included.
 *   2 = fp32 products assembled from six bf16 products of three-way split operands (x = x1 + x2 + x3 exactly,
 *       a*b = a1b1 + a2b1 + a1b2 + a2b2 + a1b3 + a3b1, fp32 accumulation) on v_mfma_f32_32x32x16_bf16 -- the direct kernel
 *       conv_x3.hip, forward and data gradient; error against fp64 = an fp32 direct convolution's (tests); in eval the
 *       decoder's bilinear x2 is fused into the full-resolution layers.  Storage, the other kernels and the weight gradients
 *       are unchanged (fp32).
 *   0 = v_mfma_f32_32x32x2_f32 (fp32 operands) throughout: Winograd F(2x2,3x3) / direct kernels (the round-1/2 default).
 *   1 = bf16 MFMA operands (configs[4] arithmetic): the Winograd convolutions (forward, data gradient, weight gradient) and
 *       the 1x1 weight-gradient GEMM round their operands to bf16 (RNE, in registers); accumulation, every stored tensor, the
 *       master weights and Adam stay fp32.   -1 = back to the handle's default (3, or VR_MFMA_MODE).
 * "mfma_bf16": 1 = "mfma_mode" 1; 0 = back to the handle's default mode.
 * "params_dirty": the parameter arena was written from outside (vr_param_arena).
 * "conv_x3d" (round 6, "mfma_mode" 3 only): the 16-column layers of 256-frame crops -- the ASPP branch convs (lib/layers.py:74-85) and
 *   Encoder.conv2 of enc5 -- on the fp16 matrix pipe: 2 (default, also -1) with the four ASPP branches of a module in one launch,
 *   1 one launch per conv, 0 the fp32-pipe kernels.
 * "conv_x3s" ("mfma_mode" 3 only, eval): the encoders' 3x3 stride-2 convs (Encoder.conv1, lib/layers.py:33) with at least 32 output
 *   columns and more than 16 input channels on the fp16 matrix pipe: 1 (default, also -1; VR_CONV_X3S=0 makes 0 the default),
 *   0 the fp32-pipe kernel for them.
 * "aspp_pool_fused" (eval, default 1): where the four ASPP branch convs of a module go out as one launch ("conv_x3d" 2), the module's
 *   pooled branch (the mean over frequency and its 1x1 Conv2DBNActiv, lib/layers.py:72-73) is a fifth part of that launch; 0 = its two
 *   launches of before.
 * "lstm_gemm" (eval, default 1, every "mfma_mode"): the LSTM input projection and the Linear behind the LSTM (lib/layers.py:117-121) as
 *   rows_gemm launches (fp32 matrix instructions); 0 = the one-row 1x1 conv launches of before.
 * "complex_train" (default 0; VR_CREATE_COMPLEX handles only, VR_ERR_BAD_ARGUMENT on a magnitude handle): 1 = the training entry points
 *   take this complex-mask handle (see vr_create_ex); 0 = they refuse it again.  Eval-mode calls are the same either way.   */
int vr_set_option(vr_handle h, const char* name, int value);

/* The loss vr_train_step and vr_validate_step compute on this handle (vr_forward_train / vr_backward are unchanged: there the caller
 * owns the loss).  VR_LOSS_L1 is the default and what every handle did before this function existed, bit for bit.
 * VR_LOSS_MAG_L1_WAVE_SDR is the loss the reference keeps commented out in train.py:83-88 and 125-129, with p = mask * X:
 *     loss = mean | |y| - |p| |  +  sdr_weight * sdr,     sdr = -<to_wave(y), to_wave(p)> / (||to_wave(y)|| ||to_wave(p)|| + 1e-8)
 * to_wave = torch.istft with a periodic Hann window over all B*2 signals (train.py:37-43), inner product and norms over the whole
 * batch (train.py:46-50); sdr_weight is 0.01 there.  In eval, vr_validate_step computes the same on p = predict(X) and
 * crop_center(y).  Every gradient term carries 1 / accumulation_steps; the gradient of | |y| - |p| | is 0 where |p| = 0 and where
 * the two magnitudes are equal.  Under data parallelism the sdr is per rank over that rank's batch (N ranks == gradient accumulation).
 * Kind 1 is accepted only on a VR_CREATE_COMPLEX handle whose option "complex_train" is on (torch.istft rejects real input) and only
 * where hop_length * 2 == n_fft (128 <= n_fft <= 4096: the tiled signal kernels); anything else returns VR_ERR_BAD_ARGUMENT before the
 * device is touched, and vr_last_error says which condition failed.  vr_set_option(h, "complex_train", 0) puts the loss back to
 * VR_LOSS_L1.  sdr_weight is ignored for kind 0 (vr_get_loss then reports 0.01).
 * vr_loss_terms: the two terms of the last vr_train_step / vr_validate_step under kind 1 on this handle, unweighted: mean | |y| - |p| |
 * and sdr (VR_ERR_BAD_ARGUMENT when there has been none since the loss was set).                                                    */
#define VR_LOSS_L1               0   /* today's loss, the default */
#define VR_LOSS_MAG_L1_WAVE_SDR  1
/* VR_LOSS_MAG_L1_WAVE_WSDR: the same with the reference's weighted_sdr_loss (train.py:53-65) as the wave term.  With xw = to_wave(X),
 * yw = to_wave(y), pw = to_wave(p), the residuals n = xw - yw and q = xw - pw sample by sample, eps = 1e-8, sums over the whole batch:
 *     loss = mean | |y| - |p| |  +  sdr_weight * wsdr,     wsdr = -(alpha * y_sdr + (1 - alpha) * noise_sdr)
 *     y_sdr = <yw, pw> / (||yw|| ||pw|| + eps),  noise_sdr = <n, q> / (||n|| ||q|| + eps),  alpha = <yw, yw> / (<yw, yw> + <n, n> + eps)
 * In eval, vr_validate_step computes it on p = predict(X), crop_center(y) and crop_center(X).  It is accepted and refused where kind 1
 * is, is put back to VR_LOSS_L1 by "complex_train" 0, and scales its gradient the same way.  vr_loss_terms then gives mean | |y| - |p| |
 * and wsdr; vr_loss_terms_wsdr gives y_sdr, noise_sdr and alpha of the last step under this kind (VR_ERR_BAD_ARGUMENT when there has
 * been none since the loss was set).
 * The value is 3: kind 2 is not a loss of this library and stays refused with VR_ERR_BAD_ARGUMENT (callers and tests rely on
 * vr_set_loss(h, 2, ...) failing with "kind" in vr_last_error).                                                                       */
#define VR_LOSS_MAG_L1_WAVE_WSDR 3
int vr_set_loss(vr_handle h, int kind, double sdr_weight);
int vr_get_loss(vr_handle h, int* kind, double* sdr_weight);
int vr_loss_terms(vr_handle h, double* mag_l1, double* sdr);
int vr_loss_terms_wsdr(vr_handle h, double* y_sdr, double* noise_sdr, double* alpha);

/* CascadedNet.forward (mode 0) / predict_mask (mode 1) / predict (mode 2)   lib/nets.py:82-141
 * x:   [B, 2, n_fft/2+1, T] fp32 magnitudes (a VR_CREATE_COMPLEX handle: complex64, and out complex64)
 * out: mode 0 [B,2,bins,T];  modes 1,2 [B,2,bins,T-128]                                          */
int vr_forward(vr_handle h, const float* x, int x_on_device, int B, int T, int mode, float* out,
               int out_on_device);

/* spec_utils.wave_to_spectrogram(wave, hop_length, n_fft)          lib/spec_utils.py:26-31
 * wave [2, L] -> spec [2, bins, 1 + L/hop] complex64                                              */
int vr_stft(vr_handle h, const float* wave, int wave_on_device, int64_t L, float* spec, int spec_on_device);

/* spec_utils.spectrogram_to_wave(spec, hop_length)                 lib/spec_utils.py:157-165
 * spec [2, bins, T] -> wave [2, hop*(T-1)]                                                        */
int vr_istft(vr_handle h, const float* spec, int spec_on_device, int T, float* wave, int wave_on_device);

/* Separator(model, device, batchsize, cropsize).separate / separate_tta     inference.py:70-102
 * spec [2,bins,T] complex64 -> y_spec (instruments), v_spec (vocals), same shape.
 * `tta` is a flag word: bit 0 = --tta (separate_tta), bit 1 = --postprocess (spec_utils.merge_artifacts,
 * lib/spec_utils.py:60-93, inference.py:27-30).
 * This, vr_separate_wave and vr_separate_pcm are the many-songs call below with one song (one executor).  batchsize counts crops of
 * the song's crop list -- pass 0, then for --tta pass 1, so the two passes may share a device batch -- and is capped at the crops
 * of the longer pass, T / roi + 1 (+ 1 with --tta), roi = cropsize - 2 * offset; batchsize <= 0 means that cap: all crops of a
 * pass in one device batch, never more.  Errors of these three name no song. */
int vr_separate(vr_handle h, const float* spec, int spec_on_device, int T, int tta, int batchsize,
                int cropsize, float* y_spec, float* v_spec, int out_on_device);

/* The whole of inference.py:147-176 in one device-resident call:
 * wave_to_spectrogram -> Separator.separate[_tta] -> spectrogram_to_wave x2.
 * wave [2, L] -> y_wave, v_wave [2, hop*(L/hop)]                                                  */
int vr_separate_wave(vr_handle h, const float* wave, int wave_on_device, int64_t L, int tta, int batchsize,
                     int cropsize, float* y_wave, float* v_wave, int out_on_device);

/* ---- WAV sample bytes in, PCM16 stems out: the file's encoding handled by the first and the last kernel -----------------
 * What python -m vocal_remover_amd.inference did on the host around vr_separate_wave -- audio._decode (interleaved PCM -> planar
 * float32) in front, audio.write's clip(rint(x * 32767)) behind -- done where the samples pass through registers anyway: the STFT
 * reads the file's bytes, the masked iSTFT writes the file's bytes.  No extra pass, no extra launch, and the transfers carry the
 * file's sample size instead of float32.  The arithmetic is csrc/pcm.h, compiled for both sides:
 *   in   `bytes`: `frames` interleaved frames of `channels` (1 or 2) samples in format `fmt`:
 *          VR_PCM_S16  v / 32768            VR_PCM_S24  little-endian, sign-extended, / 2^23
 *          VR_PCM_S32  (float)((double)v / 2^31)       VR_PCM_F32  IEEE float32 as stored
 *        -- bit for bit the float32 audio._decode produces.  One channel: both network channels read the one sample
 *        (inference.py:143-145).  8-bit PCM and float64 files stay on the host path.
 *   out  int16 [samples][2] interleaved: clip(rint(x * 32767), -32768, 32767), round-half-even, of the very float the float entry
 *        point would have stored; +-inf clip, NaN gives 0.
 * Alignment: a VR_PCM_S24 buffer may start at any byte (the kernel reads aligned 32-bit words and assembles straddling samples in
 * registers); DEVICE buffers of VR_PCM_S16 / S32 / F32 need their natural alignment and device int16 outputs 2 bytes, else
 * VR_ERR_BAD_ARGUMENT (host buffers are copied through the staging arena and may lie anywhere).
 * Only the frame-tiled kernels have these forms.  vr_pcm_available says whether the handle has them: hop_length == n_fft / 2 (every
 * reference call site), n_fft >= 128 and small enough for the tile to fit the LDS budget, VR_NO_TILED_STFT unset.  Without them
 * every call below is VR_ERR_BAD_ARGUMENT with the reason, and the caller converts on the host as before.  Host buffers are staged in the handle's
 * staging arena (vr_arena_bytes): no allocation per call once it has grown.
 *   vr_stft_pcm          vr_stft of the decoded bytes: spec [2, bins, 1 + frames / hop]
 *   vr_istft_pcm16       vr_istft, encoded: out [hop * (T - 1)][2]
 *   vr_separate_pcm      vr_separate_wave with bytes at both ends: y, v int16 [hop * (frames / hop)][2]
 *   vr_separate_pcm_many vr_separate_wave_many likewise, format and channel count per song
 *   vr_pcm_convert_host / vr_pcm16_from_float_host   the same header compiled for the host, no handle, no GPU: planar_out
 *        [channels][frames] float32 (any alignment of `bytes`); out[i] = the encoding of x[i]                                   */
enum vr_pcm_format { VR_PCM_S16 = 1, VR_PCM_S24 = 2, VR_PCM_S32 = 3, VR_PCM_F32 = 4 };
int vr_pcm_available(vr_handle h, int* available);
int vr_stft_pcm(vr_handle h, const void* bytes, int on_device, int64_t frames, int channels, int fmt, float* spec, int spec_on_device);
int vr_istft_pcm16(vr_handle h, const float* spec, int on_device, int T, int16_t* out, int out_on_device);
int vr_separate_pcm(vr_handle h, const void* bytes, int on_device, int64_t frames, int channels, int fmt, int tta, int batchsize,
                    int cropsize, int16_t* y, int16_t* v, int out_on_device);
int vr_separate_pcm_many(vr_handle h, int n_songs, const void* const* bytes, int on_device, const int64_t* frames, const int* channels,
                         const int* fmt, int tta, int batchsize, int cropsize, int16_t* const* y, int16_t* const* v, int out_on_device);
int vr_pcm_convert_host(int fmt, const void* bytes, int64_t frames, int channels, float* planar_out);
int vr_pcm16_from_float_host(const float* x, int64_t n, int16_t* out);

/* ---- many songs in one call: what pseudo.py:40-74 (a dataset) and a folder of inputs do one file at a time ------------
 * Separator.separate[_tta] for n_songs spectrograms of different lengths in ONE call.
 * specs[s]: [2,bins,T[s]] complex64; y_specs[s], v_specs[s]: same shape.  tta (flag word) / cropsize as vr_separate.
 * The result for song s is what vr_separate returns for that song alone: its own normaliser, its own make_padding, its own
 * merge_artifacts runs.  What the songs share is the device batches: the crops of all songs, and of both --tta passes, form one list
 * and batchsize counts crops of that list (<= 0: every crop of the call in one batch), so a short clip no longer pays the
 * network's launch-bound tails for two crops of its own.  Front end and back end are one launch each for all songs.
 * Magnitude and VR_CREATE_COMPLEX handles.  n_songs == 1 is valid.  One stream drain per call (one more with --postprocess).
 * Errors: n_songs <= 0, a null table (both reported before the handle is looked at), a null entry, T[s] <= 0, L[s] < hop_length,
 * training mode -> VR_ERR_BAD_ARGUMENT before the device is touched; a --postprocess failure of one song (VR_ERR_INDEX, the
 * reference's IndexError) fails the call, vr_last_error() starts with "song <s>: ", no output is defined, the handle stays usable. */
int vr_separate_many(vr_handle h, int n_songs, const float* const* specs, int specs_on_device, const int* T, int tta, int batchsize,
                     int cropsize, float* const* y_specs, float* const* v_specs, int out_on_device);
/* inference.py:147-176 for n_songs waves: waves[s] [2,L[s]] -> y_waves[s], v_waves[s] [2, hop*(L[s]/hop)], as vr_separate_wave
 * gives them for each song alone.  The pointer tables themselves are host memory; `*_on_device` describe what they point to. */
int vr_separate_wave_many(vr_handle h, int n_songs, const float* const* waves, int waves_on_device, const int64_t* L, int tta,
                          int batchsize, int cropsize, float* const* y_waves, float* const* v_waves, int out_on_device);

/* ---- spectrogram images: lib/spec_utils.py:34-57 on the device ------------------------------------
 * spectrogram_to_image in float32 as numpy evaluates it: y = log10(|z|^2 + 1e-8) (VR_IMAGE_MAGNITUDE; a float input: s^2) or angle(z)
 * (VR_IMAGE_PHASE; a float input: s), lo = min y, r = max (y - lo), pixel = uint8((y - lo) * (255 / r)), truncated.
 * vr_spec_image_many: specs[i] [channels][bins][T[i]] complex64 (is_complex) or float32 -> imgs[i]: channels == 2 gives
 * [bins][T[i]][3] bytes = (max(L, R), L, R), channels == 1 gives [bins][T[i]]; no vertical flip, the input is not modified.  ranges
 * (HOST, may be null) [n][2] = (lo, r) of every picture.  One range launch and one write launch cover all n pictures; no handle.
 * A constant input (r == 0; the reference casts NaN to uint8 there) gives a picture of zeros.  NaN or Inf in the input: the picture is
 * unspecified, nothing outside it is touched.  Device inputs need their natural alignment (8 / 4 bytes); pictures may lie anywhere.
 * vr_separate_wave_many_img / vr_separate_pcm_many_img: the call without the suffix, which also returns for every song the magnitude
 * pictures y_img[s], v_img[s] [bins][1 + L[s] / hop][3] of the instruments and vocals spectrograms -- of the very values
 * vr_separate_many would have stored, formed from the resident spectrogram and mask: no stem spectrogram is stored for them.  The
 * pictures lie where the stems lie (out_on_device).  ranges (HOST, may be null) [n_songs][2 stems][2].  The stems are bit for bit
 * those of the call without the suffix; BOTH stem tables null: pictures only, no stem is formed.
 * Errors (VR_ERR_BAD_ARGUMENT, the device untouched): n <= 0, a null table or entry, channels not 1 or 2, bins or T[i] <= 0, more
 * than 2^31 - 1 pixels in a picture, an unknown mode, one picture table or one stem table null and the other not, training mode.   */
enum vr_image_mode { VR_IMAGE_MAGNITUDE = 0, VR_IMAGE_PHASE = 1 };
int vr_spec_image_many(int device, int n, const void* const* specs, int on_device, int channels, int bins, const int* T, int is_complex,
                       int mode, uint8_t* const* imgs, int out_on_device, float* ranges /* [n][2] or null */);
int vr_spec_image(int device, const void* spec, int on_device, int channels, int bins, int T, int is_complex, int mode, uint8_t* img,
                  int out_on_device, float* range /* [2] or null */);
int vr_separate_wave_many_img(vr_handle h, int n_songs, const float* const* waves, int waves_on_device, const int64_t* L, int tta,
                              int batchsize, int cropsize, float* const* y_waves, float* const* v_waves, int out_on_device,
                              uint8_t* const* y_img, uint8_t* const* v_img, float* ranges /* [n_songs][2 stems][2] or null */);
int vr_separate_pcm_many_img(vr_handle h, int n_songs, const void* const* bytes, int on_device, const int64_t* frames, const int* channels,
                             const int* fmt, int tta, int batchsize, int cropsize, int16_t* const* y, int16_t* const* v, int out_on_device,
                             uint8_t* const* y_img, uint8_t* const* v_img, float* ranges /* [n_songs][2 stems][2] or null */);

/* ---- score a separation against the true stems: windowed SDR sums on the device -----------------
 * vr_separate_wave_many that also measures each song.  mix[s], inst[s]: float32 [2, L[s]], the mixture and its true instruments (both
 * on the host or both on the device, `on_device`).  With samples = hop * (L / hop), the stems y, v of vr_separate_wave and the true stems
 * r_y = inst[:, :samples], r_v = (mix - inst)[:, :samples], window w covers samples [w * window, min((w + 1) * window, samples)) of both
 * channels, n_windows = ceil(samples / window), and
 *     sums[s][w] = { sum r_y^2, sum (r_y - y)^2, sum r_v^2, sum (r_v - v)^2 }            (HOST doubles, [n_windows][4])
 * Every term is formed and added in double from the float32 samples; the estimate is the very float the stem holds (or would hold).
 * The library returns sums, not decibels, and hides no epsilon: sdr = 10 log10(sums[.][0] / sums[.][1]) per window, from the column
 * sums for the whole song (spec_utils.sdr_from_sums).  Two identical calls give bit-identical sums: no atomics, a fixed order.
 * y_waves / v_waves: the stems as vr_separate_wave_many returns them, or BOTH tables null: sums only -- no stem is then allocated,
 * stored or copied.  window >= hop_length (44100 = one second of the reference's audio).  tta (flag word) / batchsize / cropsize as
 * vr_separate_wave_many.  Magnitude and VR_CREATE_COMPLEX handles; float waves only (no sample bytes, no PCM16 stems, no streams), and
 * only where hop_length == n_fft / 2 -- the sums are formed in the frame-tiled masked iSTFT kernel, which exists only there.
 * Errors (VR_ERR_BAD_ARGUMENT, the device untouched): n_songs <= 0, a null table, one stem table null and the other not (these before
 * the handle is looked at); a null entry, L[s] < hop_length, window < hop_length, another hop, training mode.  Errors of a many-call
 * start with "song <s>: " where they concern one song.
 *   vr_evaluate_wave     the many-call of one song (`solo` as for vr_separate_wave: batchsize <= 0 = the crops of its longer pass);
 *                        y_wave and v_wave both null: sums only
 *   vr_evaluate_plan     no handle, no device: samples and n_windows of a song of L samples (L < hop or window < hop: VR_ERR_BAD_ARGUMENT) */
int vr_evaluate_wave_many(vr_handle h, int n_songs, const float* const* mix, const float* const* inst, int on_device, const int64_t* L, int tta,
                          int batchsize, int cropsize, int64_t window, double* const* sums, float* const* y_waves, float* const* v_waves,
                          int out_on_device);
int vr_evaluate_wave(vr_handle h, const float* mix, const float* inst, int on_device, int64_t L, int tta, int batchsize, int cropsize,
                     int64_t window, double* sums, float* y_wave, float* v_wave, int out_on_device);
int vr_evaluate_plan(int hop, int64_t L, int64_t window, int64_t* samples, int64_t* n_windows);

/* ---- pseudo-instrument labels (the reference's pseudo.py:40-74), many pairs in one call ------------------------------------------------
 * For pair s of a mixture X_s and its imperfect instrumental y_s, both complex64 [2][bins][T_s]:
 *     D_s = X_s - y_s                                   (one float32 subtraction per component, as numpy's complex64 difference)
 *     a_s = instruments stem of vr_separate of D_s      (flag word `tta` as vr_separate: bit 0 --tta, bit 1 --postprocess)
 *     P_s = y_s + a_s                                   (one float32 addition per component, never contracted with the product before it)
 * out[s] receives P_s, T_s frames of complex64, as [2][bins][T] (VR_PSEUDO_SPEC, what pseudo.py saves) or as [T][2][bins]
 * (VR_PSEUDO_ROWS, the rows of the training cache: vr_dataset_add takes them as they are).  Nothing else is stored or copied: no vocal
 * stem, no wave, and at wave level not X either.  Each pair comes out as it would alone -- the normaliser is that of D_s (max|D|, or for tta
 * the lexicographic complex maximum), padding and merge_artifacts runs are its own -- while the crops of all pairs and of both passes share
 * device batches exactly as in vr_separate_many.  A pair with X == y everywhere has D = 0 and gives what vr_separate_many gives for a zero
 * spectrogram (the reference divides 0 by 0 there: NaN); it is not treated specially.  pseudo.py always runs tta; the flag is honoured.
 *   vr_pseudo_many        mix_specs[s], inst_specs[s]: [2][bins][T[s]] complex64 (both tables on the host or both on the device); any hop_length
 *   vr_pseudo_wave_many   mix_waves[s], inst_waves[s]: float32 [2][L[s]], already aligned, the same length; T = 1 + L / hop as for vr_stft.  One
 *                         launch transforms both waves of all pairs (the pair form of the frame-tiled STFT), so it exists only where
 *                         hop_length == n_fft / 2; elsewhere VR_ERR_BAD_ARGUMENT with the reason
 *   vr_pseudo, vr_pseudo_wave   the many-call of one pair (`solo` as for vr_separate: batchsize <= 0 = the crops of its longer pass)
 * Magnitude and VR_CREATE_COMPLEX handles.  Errors as for vr_separate_many: n_songs <= 0, a null table or an unknown layout before the
 * handle is looked at; a null entry, T[s] <= 0, L[s] < hop_length or training mode before the device is touched; errors of a many-call
 * that concern one pair start with "song <s>: ", a solo call's name no song; a --postprocess IndexError of one pair fails the call with
 * VR_ERR_INDEX and leaves the handle usable.                                                                                        */
enum vr_pseudo_layout { VR_PSEUDO_SPEC = 0 /* [2][bins][T], pseudo.py's .npy */, VR_PSEUDO_ROWS = 1 /* [T][2][bins], the cache's */ };
int vr_pseudo_many(vr_handle h, int n_songs, const float* const* mix_specs, const float* const* inst_specs, int on_device, const int* T, int tta,
                   int batchsize, int cropsize, int layout, float* const* out, int out_on_device);
int vr_pseudo_wave_many(vr_handle h, int n_songs, const float* const* mix_waves, const float* const* inst_waves, int on_device, const int64_t* L,
                        int tta, int batchsize, int cropsize, int layout, float* const* out, int out_on_device);
int vr_pseudo(vr_handle h, const float* mix_spec, const float* inst_spec, int on_device, int T, int tta, int batchsize, int cropsize, int layout,
              float* out, int out_on_device);
int vr_pseudo_wave(vr_handle h, const float* mix_wave, const float* inst_wave, int on_device, int64_t L, int tta, int batchsize, int cropsize,
                   int layout, float* out, int out_on_device);

/* ---- pitch-shifted waves and training pairs (the reference's augment.py), many per call ---------------------------------------------------
 * The shift of one signal y of L samples is librosa.effects.pitch_shift's, not SoundTouch's (DESIGN.md section 6r says why), with
 * rate = 2 ** (-n_steps / bins_per_octave) and ratio = sr / (float(sr) / rate), both formed by the caller in double:
 *     D  = stft(y, n_fft, hop)                         periodic Hann, centre zero pad, T = 1 + L / hop
 *     D' = phase_vocoder(D, rate, hop)                 T_stretch = ceil(T / rate) frames; the phase is accumulated in double
 *     ys = istft(D', hop, length = round(L / rate))    n_stretch samples
 *     z  = fix_length(resample(ys, ratio), L)          'kaiser_fast': int(n_stretch * ratio) samples computed, n_resampled =
 *                                                      ceil(n_stretch * ratio) with the zero tail, then cut or zero-padded to L
 *   vr_pitch_plan        no handle, no device: the four lengths, from the expressions the launches use (L < n_fft: VR_ERR_BAD_ARGUMENT)
 *   vr_phase_vocoder     spec [signals][bins][T] complex64 -> out [signals][bins][ceil(T / rate)], bins and hop the handle's
 *   vr_istft_length      vr_istft with librosa's length=: wave [2][length] = the overlap-add behind the n_fft / 2 in front, cut or
 *                        followed by zeros; always the per-frame kernels, whatever the hop
 *   vr_resample_ratio    vr_resample for a ratio that is no quotient of two integer rates (vr_resample is this at (double)sr_out / sr_in)
 *   vr_pitch_shift_many  waves[i] [channels][L[i]] -> out[i] of the same shape, shifted at the handle's n_fft / hop_length
 *   vr_pitch_pair_many   mix[i], inst[i] float32 [2][L[i]], aligned: y' = shift(inst), v' = shift(mix - inst) (one float32 subtraction per
 *                        sample), X' = y' + v' (one float32 addition), the shifts at shift_n_fft / shift_hop; X_out[i] / y_out[i] = the
 *                        STFTs of X' / y' at the handle's n_fft / hop_length, T = 1 + L[i] / hop_length frames, as [2][bins][T]
 *                        (VR_PSEUDO_SPEC) or [T][2][bins] (VR_PSEUDO_ROWS: hop_length == n_fft / 2 only).  The pair's peak
 *                        max(max|X'|, max|y'|) is not an output: the caller takes it from the stored values, as for every cache
 * The items of a call run one after the other through one workspace, sized for the largest item: its spectrogram at the shift's hop, the
 * stretched one and the inverse transform's frames, about 210 bytes per sample of a pair at 2048 / 512 and rate near 1 (1.7 GB for 180 s at 44.1 kHz).  It is checked against max_bytes
 * (<= 0: nine tenths of the free device memory) before anything is allocated: VR_ERR_OOM, and vr_last_error() names both sizes.  Nothing
 * is accumulated with atomics: two identical calls agree bit for bit.                                                                */
int vr_pitch_plan(int64_t L, int n_fft, int hop, double rate, double ratio, int* T, int* T_stretch, int64_t* n_stretch, int64_t* n_resampled);
int vr_phase_vocoder(vr_handle h, const float* spec, int on_device, int signals, int T, double rate, float* out, int out_on_device);
int vr_istft_length(vr_handle h, const float* spec, int spec_on_device, int T, int64_t length, float* wave, int wave_on_device);
int vr_resample_ratio(int device, const float* x, int channels, int64_t n_in, double ratio, float* y, int64_t n_out);
int vr_pitch_shift_many(vr_handle h, int n, const float* const* waves, int on_device, int channels, const int64_t* L, double rate, double ratio,
                        int64_t max_bytes, float* const* out, int out_on_device);
int vr_pitch_pair_many(vr_handle h, int n, const float* const* mix, const float* const* inst, int on_device, const int64_t* L, int shift_n_fft,
                       int shift_hop, double rate, double ratio, int layout, int64_t max_bytes, float* const* X_out, float* const* y_out,
                       int out_on_device);

/* ---- plain training pairs on the device: trim, align, STFT rows and peak, many pairs per call (csrc/prepare.hip) ----
 * What the reference's spec_utils.cache_or_load does to a decoded (mixture, instrumental) pair, in two steps; the window of step 1
 * sizes the outputs of step 2, so it comes back to the host between them (64 bytes per pair).  Waves are float32 [2][L], host or device.
 *   vr_pair_window_plan  no device: the window arithmetic, the one statement every layer uses.  lag > 0 moves a_off = a_start + lag, otherwise
 *                        b_off = b_start - lag; n = min(a_end - a_off, b_end - b_off); n <= 0 is VR_ERR_BAD_ARGUMENT.
 *   vr_align_pair_many   no handle.  Per wave librosa.effects.trim(top_db 60, frame_length 2048, hop_length 512): centre zero padding of
 *                        1024 samples, 1 + L / 512 frames, per frame and channel the mean square summed in double and rms =
 *                        float32(sqrt(.)), ref = the largest rms of both channels, a frame is signal where on any channel
 *                        20 log10(max(1e-5, rms)) - 20 log10(max(1e-5, ref)) > -60; start = first * 512, end = min(L, (last + 1) * 512)
 *                        (an all-zero wave keeps everything).  Heads: the first min(4 * sr, end - start) trimmed samples, the two channels
 *                        added (one float32 addition), the mean (summed in double) removed.  lag = argmax_first(correlate(a, b, 'full')) -
 *                        (na - 1), correlation and argmax on the device; the contract of the lag search is the lag of a well-conditioned
 *                        pair, not the bits of the correlation (vr_xcorr_argmax keeps its own arithmetic).  Every stage but the
 *                        correlation is one launch over the call's table; one wait and one copy of n windows back per call.  An empty
 *                        window is VR_ERR_BAD_ARGUMENT and vr_last_error() names the pair.  inst[i] NULL: the mixture is trimmed alone
 *                        (b_start, b_end repeat a_start, a_end; no correlation, lag 0).
 *   vr_pair_rows_many    the STFT rows [T][2][bins] complex64 (the training cache's layout, T = 1 + n / hop_length) of
 *                        mix[i][:, a_off : a_off + n] and inst[i][:, b_off : b_off + n] at the handle's n_fft / hop_length, the values those of
 *                        vr_stft on the sliced waves, and peaks[i] = max(max|X|, max|y|) as numpy forms it in float32, taken on the device
 *                        from the rows just written.  The windows are the caller's: however they were found.  hop_length != n_fft / 2:
 *                        VR_ERR_UNSUPPORTED (the rows are a form of the frame-tiled STFT).  The pairs run one after the other through one
 *                        workspace sized for the largest (its two windows, and the rows when the outputs are host memory), checked against
 *                        max_bytes (<= 0: nine tenths of the free device memory) before anything is allocated: VR_ERR_OOM, and
 *                        vr_last_error() names both sizes.
 * Nothing is accumulated with atomics: two identical calls agree bit for bit.                                                         */
typedef struct vr_pair_window {
    int64_t a_start, a_end;     /* the mixture's trimmed range */
    int64_t b_start, b_end;     /* the instrumental's */
    int64_t lag;                /* > 0: the mixture starts late by lag samples */
    int64_t a_off, b_off, n;    /* the common window: n samples from a_off of the mixture, from b_off of the instrumental */
} vr_pair_window;
int vr_pair_window_plan(int64_t a_start, int64_t a_end, int64_t b_start, int64_t b_end, int64_t lag, vr_pair_window* out);
int vr_align_pair_many(int device, int n, const float* const* mix, const float* const* inst, int on_device, const int64_t* L_mix,
                       const int64_t* L_inst, int sr, vr_pair_window* out);
int vr_pair_rows_many(vr_handle h, int n, const float* const* mix, const float* const* inst, int on_device, const int64_t* L_mix,
                      const int64_t* L_inst, const vr_pair_window* w, int64_t max_bytes, float* const* X_out, float* const* y_out,
                      int out_on_device, float* peaks);

/* ---- streaming separation: push audio in blocks, get the stems back with bounded state -----------------------------------
 * The offline call's crops sit at multiples of roi = cropsize - 2 * offset whatever the song's length (make_padding: pad_l = offset),
 * the --tta pass is the same list shifted by roi / 2, and with hop == n_fft / 2 frame t needs the samples below (t + 1) * hop.  The
 * only whole-song quantity is the normaliser c.  GIVEN c, a stream therefore runs the crops vr_separate_wave runs, on the same numbers:
 * for any split of a wave [2][L] into pushes of any sizes >= 1 followed by vr_stream_flush, the concatenated y / v have hop * (L / hop)
 * samples and are what vr_separate_wave(tta = flags & VR_STREAM_TTA) returns for the whole wave on this handle (the batches are
 * composed differently, which moves the result by rounding only: tests hold 2e-4 * scale, the bar between the offline entry points),
 * provided (coef_re, coef_im) is that call's normaliser: max|X| (plain; coef_im 0) or numpy's lexicographic complex maximum (tta).
 * A magnitude handle uses |coef|, a VR_CREATE_COMPLEX handle the complex number (both kinds of handle are supported).  A
 * VR_STREAM_MEASURE stream runs no network and returns no samples; after its flush vr_stream_coef gives exactly that normaliser
 * (the lexicographic maximum with VR_STREAM_TTA, else max|X| and 0), from the statistics pass of the offline path.
 * coef_re == coef_im == 0 (plain streams only; with VR_STREAM_TTA it is VR_ERR_BAD_ARGUMENT): a RUNNING normaliser -- crop i is
 * divided by max|X| over the frames below (i + 1) * roi + offset, the end of its own window.  That is NOT the offline result (it is,
 * when the loudest frame lies inside crop 0's window); like every mode it does not depend on how the input was split into pushes.
 * Zero padding in front of the first and behind the last frame, the right zero padding of the last crops and the window-sum division
 * are the offline kernels'.  A frame whose window reaches past the samples received waits for more data or for the flush.
 *
 * vr_stream_push runs every crop that has become ready -- the crops of both passes share device batches of `batchsize` (<= 0: 8) --
 * and returns every output sample that is final: *n_out per channel, possibly 0, at y / v [2][capacity] (channel pitch = capacity).
 * A capacity below what the call returns is VR_ERR_BAD_ARGUMENT, reported before anything is consumed; vr_last_error() names the size
 * needed (vr_stream_plan computes it: samples_out after minus before).  wave: planar [2][n].
 * vr_stream_info: lookahead_samples = (roi + offset) * hop (VR_STREAM_POSTPROCESS: (roi + offset + 161) * hop), the samples that must have arrived before the first output sample;
 * block_samples = roi * hop, the step in which crops become ready; state_bytes = the device memory the stream holds: an input tail,
 * a ring of spectrogram frames, a mask ring per pass, one hop of overlap-add carry per stem and channel, the normaliser.  It depends
 * on (n_fft, cropsize, batchsize, flags) and not on how much audio has passed; the handle's staging arena holds one push (see
 * vr_arena_bytes).  A push larger than batchsize * roi frames is worked through in steps of that size.
 * VR_STREAM_POSTPROCESS: the stream applies spec_utils.merge_artifacts (thres 0.05, min_range 64, fade_size 32, as vr_separate_wave's
 * postprocess) to its mask.  The blend weight of frame t is final once the mask minima of the frames below t + 161 are known (161 =
 * 3 * fade_size + min_range + 1), so such a stream returns its samples 161 frames later -- lookahead_samples = (roi + offset + 161) * hop --
 * keeps that many more frames and mask columns plus a ring of minima, a ring of weights and five ints, and a steady push adds two small
 * launches (the minima, the walk over them); at flush everything left is final.  The concatenated stems are what vr_separate_wave with
 * postprocess returns, at the same bar.  One deviation: a song with no frame above the threshold is an error offline (the reference's
 * IndexError); a stream has returned samples before that could be known, never raises for it, and blends nothing.  With a given
 * normaliser it combines with every other flag and entry point; VR_STREAM_MEASURE (no samples) and the running normaliser refuse it.
 * Errors (VR_ERR_BAD_ARGUMENT, before the device is touched): training mode (at open and at every push), hop_length != n_fft / 2,
 * VR_STREAM_POSTPROCESS with VR_STREAM_MEASURE or coef 0, an unknown flag, push or flush after flush, fewer than hop_length
 * samples in all at flush ("wave shorter than one hop", as vr_separate_wave).  Other calls on the handle between two pushes are
 * allowed (the stream keeps nothing in the handle's arenas); a stream must be closed before its handle is destroyed.  A push that
 * fails half way (a HIP error) leaves the stream unusable: close it. */
typedef struct vr_stream_s* vr_stream;
#define VR_STREAM_TTA         1   /* second pass shifted by roi/2, masks averaged (separate_tta)                  */
#define VR_STREAM_MEASURE     2   /* no network, no output: only accumulate the normaliser                        */
#define VR_STREAM_POSTPROCESS 4   /* merge_artifacts with 161 frames of look-ahead: see above                     */
/* y / v of vr_stream_push, vr_stream_flush and vr_stream_push_many are int16 [capacity][2] interleaved (pass them cast to float*):
 * the encoding of vr_separate_pcm of the very floats the stream would have returned.  capacity and n_out still count samples per
 * channel; the input stays planar float.  All streams of one vr_stream_push_many call must agree on it (VR_ERR_BAD_ARGUMENT).   */
#define VR_STREAM_PCM16_OUT   8
int vr_stream_open(vr_handle h, int cropsize, int batchsize, int flags, double coef_re, double coef_im, vr_stream* out);
int vr_stream_push(vr_stream s, const float* wave, int on_device, int64_t n, float* y, float* v, int out_on_device, int64_t capacity,
                   int64_t* n_out);
int vr_stream_flush(vr_stream s, float* y, float* v, int out_on_device, int64_t capacity, int64_t* n_out);
/* Many streams of ONE handle in one call: stream k receives n[k] >= 0 more samples (wave[k], planar [2][n[k]]) and, where flush[k] != 0,
 * its input ends there (a push followed by a flush; flush == NULL: no stream ends).  n[k] == 0 without flush leaves stream k untouched.
 * y[k] / v[k]: [2][capacity[k]]; n_out[k] = the final samples returned, exactly vr_stream_plan's samples_out after minus before.
 * CONTRACT: the samples stream k returns and its state afterwards are what vr_stream_push (then vr_stream_flush) on that stream alone
 * would have produced -- the same steps, the same crops; the bar is 2e-4 * scale as between the other entry points (a device batch
 * composed differently may change a conv's tile choice).  Afterwards any stream may go on through either entry point, and other calls
 * on the handle may come between.  What the streams share is the launches: the call goes in rounds, round r = step r of every stream
 * that still has input; per round one STFT over all streams, the ready crops of all streams and both passes in shared device batches
 * of `batchsize` (independent of the batchsize a stream was opened with, which sizes its rings and its step; <= 0: the largest among
 * the streams), one masked iSTFT per stem; per call one drain.  Plain, VR_STREAM_TTA and VR_STREAM_POSTPROCESS streams may be mixed
 * (the two postprocess launches of a round serve all its streams); VR_CREATE_COMPLEX
 * handles are supported.  VR_STREAM_MEASURE streams and running-normaliser streams (coef 0) are REFUSED here: the running normaliser
 * cuts its steps per crop, which stays on vr_stream_push.
 * Checked before the device is touched, every stream left as it was (VR_ERR_BAD_ARGUMENT, vr_last_error() starts "stream <k>: "):
 * n_streams >= 1; all streams of one handle; no stream twice; equal cropsize; no stream closed (NULL), flushed or broken; eval mode;
 * capacity[k] large enough.  While the call runs its streams are marked broken, as in vr_stream_push; a call that fails half way
 * leaves them so. */
int vr_stream_push_many(int n_streams, const vr_stream* s, const float* const* wave, int on_device, const int64_t* n, const int* flush,
                        int batchsize, float* const* y, float* const* v, int out_on_device, const int64_t* capacity, int64_t* n_out);
/* The file's sample bytes into a stream: vr_stream_push / vr_stream_push_many with `bytes` = `frames` interleaved frames of `channels`
 * (1 or 2; one channel is up-mixed) samples in format `fmt` (vr_pcm_format) in place of the planar float wave.  The stream STFT reads the
 * bytes (a form of the frame-tiled kernel, csrc/pcm.h's arithmetic); no decode pass, no extra launch, and the upload carries the file's
 * sample size.  CONTRACT: each call returns exactly what the float entry point returns for vr_pcm_convert_host of the same bytes, mono
 * up-mixed -- the samples, n_out and the state left behind, bit for bit, since the first kernel sees the same floats (the input tail a
 * step keeps is stored decoded, as float32: vr_stream_info's state_bytes is unchanged).  A stream may mix float and PCM pushes freely;
 * vr_stream_flush serves both.  Every kind of stream is taken by vr_stream_push_pcm: plain, VR_STREAM_TTA, VR_STREAM_MEASURE, the running
 * normaliser, VR_STREAM_PCM16_OUT, VR_CREATE_COMPLEX handles.  vr_stream_push_many_pcm: format and channel count per stream; it refuses
 * what vr_stream_push_many refuses.  A push worked through in several steps advances through the bytes frame by frame, so a step of a
 * VR_PCM_S24 block may begin at any byte.  Host bytes are staged as bytes in the handle's staging arena, rounded up to whole 32-bit words.
 * VR_ERR_BAD_ARGUMENT, before the device or any stream is touched (vr_stream_push_many_pcm: vr_last_error() starts "stream <k>: "): an
 * unknown fmt, channels not 1 or 2, frames < 0, bytes NULL with frames > 0, a DEVICE buffer of VR_PCM_S16 / S32 / F32 off its natural
 * alignment (VR_PCM_S24 may start at any byte; host buffers may lie anywhere), and everything the float forms refuse. */
int vr_stream_push_pcm(vr_stream s, const void* bytes, int on_device, int64_t frames, int channels, int fmt, float* y, float* v,
                       int out_on_device, int64_t capacity, int64_t* n_out);
int vr_stream_push_many_pcm(int n_streams, const vr_stream* s, const void* const* bytes, int on_device, const int64_t* frames,
                            const int* channels, const int* fmt, const int* flush, int batchsize, float* const* y, float* const* v,
                            int out_on_device, const int64_t* capacity, int64_t* n_out);
int vr_stream_coef(vr_stream s, double* coef_re_im /*[2]*/);
int vr_stream_info(vr_stream s, int64_t* lookahead_samples, int64_t* block_samples, int64_t* state_bytes);
int vr_stream_close(vr_stream s);
/* Host only, no handle, no GPU: the schedule the executor follows.  After samples_in samples (flushed: and the flush):
 * frames_ready = samples_in / hop (flushed: + 1, the offline frame count); crops_ready[2] = crops run so far per pass (flushed: the
 * offline `patches` of make_padding, T / roi + 1 and, tta, T / roi + 2; crops_ready[1] = 0 without tta); samples_out = output
 * samples final so far per channel (flushed: hop * (samples_in / hop)).  Any out pointer may be NULL.
 * VR_ERR_BAD_ARGUMENT: hop * 2 != n_fft, cropsize <= 2 * offset, samples_in < 0, flushed with samples_in < hop. */
int vr_stream_plan(int n_fft, int hop, int cropsize, int offset, int tta, int64_t samples_in, int flushed, int64_t* frames_ready,
                   int64_t* crops_ready /*[2]*/, int64_t* samples_out);
/* The same with the flags of vr_stream_open in place of `tta` (VR_STREAM_TTA and VR_STREAM_POSTPROCESS matter; an unknown flag is
 * VR_ERR_BAD_ARGUMENT).  With VR_STREAM_POSTPROCESS and before the flush, samples_out counts the frames 161 below the final masks:
 * it lags vr_stream_plan's by 161 * hop once positive; flushed, both give hop * (samples_in / hop). */
int vr_stream_plan_ex(int n_fft, int hop, int cropsize, int offset, int flags, int64_t samples_in, int flushed, int64_t* frames_ready,
                      int64_t* crops_ready /*[2]*/, int64_t* samples_out);
/* Device bytes the handle holds for staging (inputs, outputs, masks of one call) and for the network's workspace. */
int vr_arena_bytes(vr_handle h, int64_t* staging_bytes, int64_t* workspace_bytes);
/* Device bytes the handle holds for the training input pipeline, a buffer of its own that vr_arena_bytes does not count: the tables and
 * host-side outputs of vr_augment_batch / vr_dataset_batch / vr_dataset_windows and, over a wave store, the STFT rows of one batch
 * (4 * B * T * 2 * bins * 8 bytes plus one eighth: about 300 MB at B 16, T 256, 1025 bins).  It grows to the largest call made and is kept
 * until the handle is destroyed, or until release != 0 here: *bytes (may be NULL) receives what was held before the call, the buffer is
 * freed after the handle's stream has drained, and the next call that needs it allocates it again. */
int vr_pipeline_buffer(vr_handle h, int64_t* bytes, int release);

/* ---- training: the body of train.train_epoch (train.py:77-96) ------------------------------------ */
/* mask = model(X); loss = L1Loss()(mask * X, y); (loss / accumulation_steps).backward()
 * X, y: [B, 2, bins, T] fp32.  Gradients ACCUMULATE in the library's gradient arena until vr_zero_grad
 * (model.zero_grad()).  *loss_out = the un-scaled mean L1 loss (loss.item()).  mask_out (optional,
 * may be NULL): the full-width mask [B,2,bins,T] that model(X) returns.  Needs vr_set_mode(h, 1).    */
int vr_train_step(vr_handle h, const float* X, const float* y, int on_device, int B, int T, int accumulation_steps,
                  float* loss_out, float* mask_out, int mask_on_device);
/* The same step as TWO calls, for callers that keep the reference's own loss expression and optimizer between them
 * (train.py:81-95 unmodified: `mask = model(X)` ... `loss.backward()` ... `optimizer.step()`):
 *   vr_forward_train   mask = model(X) under model.train(): batch-statistics BatchNorm (running buffers updated), live
 *                      Dropout2d, the graph (raw activations) kept inside the handle.  mask_out [B,2,bins,T].
 *   vr_backward        dmask = dLoss/dmask [B,2,bins,T] -> gradients ACCUMULATE in the gradient arena exactly like
 *                      vr_train_step's.  Consumes the graph; any other call on the handle in between frees it (-2).
 * vr_param_arena: the flat fp32 parameter arena (device pointer, element count; same indexing as vr_grad_arena), so
 * that an element-wise optimizer from outside (torch.optim.Adam on a zero-copy view) can update the weights in place;
 * call vr_set_option(h, "params_dirty", 1) after writing it so that eval-mode folded tables are rebuilt.            */
int vr_forward_train(vr_handle h, const float* X, int on_device, int B, int T, float* mask_out, int mask_on_device);
int vr_backward(vr_handle h, const float* dmask, int on_device);
/* Identity of the graph the handle currently holds: *generation counts the vr_forward_train calls so far, *valid (may be
 * NULL) says whether that graph is still alive.  A caller that keeps several forward results around (autograd) records the
 * generation after vr_forward_train and refuses to call vr_backward for any other one -- the handle keeps ONE graph. */
int vr_graph_generation(vr_handle h, int64_t* generation, int* valid);
int vr_param_arena(vr_handle h, float** device_ptr, int64_t* numel);

/* Training input pipeline on the device: replaces the numeric part of
 * lib/dataset.py VocalRemoverTrainingSet.__getitem__ (dataset.py:105-120) for a whole batch.
 *   X, y           [B][T][2][bins] complex64 (re,im interleaved): the cropsize rows read from the cached .npy files
 *                  (their on-disk row order; dataset.py:33-46,58-66), host or device
 *   X_mix, y_mix   the mixup partners' rows (dataset.py:85-103), same layout; may be NULL when no sample mixes
 *   desc[b]        coef (dataset.py:109), coef_mix (dataset.py:90-91), lam (np.random.beta, dataset.py:97) and flags:
 *                  bit 0 aggressively_remove_vocal, 1 channel swap, 2 inst-only, 3 mixup,
 *                  bits 4-6 = bits 0-2 for the partner (dataset.py:68-83 is applied to both independently)
 *   reduction_weight [bins]  (train.py:197-205), NULL if no flag needs it
 * Output: X_mag, y_mag [B][2][bins][T] fp32 = np.abs of the augmented crops, the tensors train_epoch consumes. */
typedef struct vr_aug { float coef; float coef_mix; float lam; int flags; } vr_aug;
int vr_augment_batch(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug* desc,
                     const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_mag, float* y_mag,
                     int out_on_device);
/* The same for a complex-mask model's batches (lib/dataset.py:120, the commented `return X, y`): everything before the final np.abs,
 * X_out, y_out [B][2][bins][T] complex64 (re,im interleaved) = the augmented crops themselves.  Any handle may call it. */
int vr_augment_batch_complex(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug* desc,
                             const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_out, float* y_out,
                             int out_on_device);

/* The extended descriptor and its entry points: two augmentations beyond lib/dataset.py's four.  vr_aug stays 16
 * bytes; vr_aug_ex is its four fields, with the same meaning, and two gains (24 bytes).  Flag bits beyond 0-6:
 *   bit 7  VR_AUG_REMIX     the partner (X_mix, y_mix of the sample; mix_song, mix_start of its vr_crop) is a REMIX partner: after
 *                           /coef_mix and the partner's swap (bit 5, its place for a mixup partner) v = X_j - y_j is the partner's
 *                           vocals, and the sample becomes y = gain_y * y, X = y + gain_v * v -- whatever inst-only made of X.  The
 *                           sample's own bits 0-2 and 8 apply first.  lam is ignored.
 *   bit 8  VR_AUG_MONO      lib/dataset.py:81-83 (commented out there), after inst-only: both channels of X and of y become
 *                           0.5f * (L + R); the two channels of the output hold the same bits.
 *   bit 9  VR_AUG_MIX_MONO  bit 8 for a mixup partner (bit 3).
 * One float32 rounding per operation written above.  The _ex entry points take what their namesakes take, check what they check and,
 * over a table in which no sample has a bit above 6, launch what they launch: the same bytes.  A remix reads the four crops a mixup
 * reads; over a wave store the scratch is what it was (vr_pipeline_buffer).  More refusals, all VR_ERR_BAD_ARGUMENT before anything is
 * launched, vr_last_error() naming the sample: bits 3 and 7 both set; bit 7 with bit 4 or 6 (a remix partner is not reduced and not
 * inst-only); bit 7 with a gain that is not finite; and, for bit 7 as for bit 3, no partner crops (vr_augment_batch_ex), mix_song < 0 or
 * the partner's rows outside its song (vr_dataset_batch_ex). */
typedef struct vr_aug_ex { float coef; float coef_mix; float lam; int flags; float gain_y; float gain_v; } vr_aug_ex;
enum { VR_AUG_MIXUP = 8, VR_AUG_REMIX = 128, VR_AUG_MONO = 256, VR_AUG_MIX_MONO = 512 };
int vr_augment_batch_ex(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug_ex* desc,
                        const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_mag, float* y_mag,
                        int out_on_device);
int vr_augment_batch_complex_ex(vr_handle h, const float* X, const float* y, const float* X_mix, const float* y_mix, const vr_aug_ex* desc,
                                const float* reduction_weight, int B, int T, int bins, int in_on_device, float* X_out, float* y_out,
                                int out_on_device);

/* The training set resident in HBM: load every song's cached spectrogram pair once, then each batch is one vr_dataset_batch -- the
 * kernel of vr_augment_batch reading the crops where they lie, no file read and no host-to-device copy of spectrogram rows.
 *   vr_dataset_create   an empty store on `device` for spectrograms of `bins` bins.  It owns its own device allocations and nothing
 *                       of any handle: it may outlive handles and serve several handles on its device.
 *   vr_dataset_add      one song: X, y host [rows][2][bins] complex64 (re,im interleaved), the on-disk layout of the cache
 *                       (spec_utils.SpectrogramCache), copied once into one device slab each.  The pointers may be memory maps of
 *                       the .npy files: the copy runs in bounded pieces through the store's own pinned staging.  *song_out (may be
 *                       NULL) is the song's index, counting from 0 in the order added.  A failed device allocation is VR_ERR_OOM,
 *                       vr_last_error() gives the bytes asked for and the bytes the store already holds; the store stays usable.
 *   vr_dataset_info     songs held, and the device bytes of their slabs.   vr_dataset_rows: the rows of one song.
 *   vr_dataset_batch    B samples of T rows: sample b is rows [start, start + T) of song crops[b].song, mixed -- when desc[b].flags has
 *                       bit 3 -- with rows [mix_start, mix_start + T) of song mix_song (both ignored otherwise).  desc,
 *                       reduction_weight and the outputs X_mag, y_mag [B][2][bins][T] are those of vr_augment_batch, and so is every
 *                       value computed.  Runs on the handle's stream and returns when the outputs are complete.
 * Errors of vr_dataset_batch, all VR_ERR_BAD_ARGUMENT and all before anything is launched (the kernel is never given a row it cannot
 * read): B <= 0 or a null table (reported before the handle and the store are looked at); a handle on another device than the store;
 * and, with vr_last_error() naming the sample: a song index out of range, start < 0, start + T > rows, the same for the partner when
 * bit 3 is set, bit 3 with mix_song < 0, bit 0 or 4 without reduction_weight. */
typedef struct vr_dataset_s* vr_dataset;
typedef struct vr_crop { int song; int mix_song; int64_t start; int64_t mix_start; } vr_crop;
int vr_dataset_create(int device, int bins, vr_dataset* out);
int vr_dataset_destroy(vr_dataset d);
int vr_dataset_add(vr_dataset d, const float* X, const float* y, int64_t rows, int* song_out);
int vr_dataset_info(vr_dataset d, int* n_songs, int64_t* bytes);
int vr_dataset_rows(vr_dataset d, int song, int64_t* rows);
int vr_dataset_batch(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug* desc, const float* reduction_weight, int B, int T,
                     float* X_mag, float* y_mag, int out_on_device);
/* vr_dataset_batch with the outputs of vr_augment_batch_complex: X_out, y_out [B][2][bins][T] complex64; same checks, same errors. */
int vr_dataset_batch_complex(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug* desc, const float* reduction_weight, int B, int T,
                             float* X_out, float* y_out, int out_on_device);
/* The two with vr_aug_ex descriptors (above): a remix partner sits in mix_song / mix_start and is checked as a mixup partner is. */
int vr_dataset_batch_ex(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug_ex* desc, const float* reduction_weight, int B, int T,
                        float* X_mag, float* y_mag, int out_on_device);
int vr_dataset_batch_complex_ex(vr_handle h, vr_dataset d, const vr_crop* crops, const vr_aug_ex* desc, const float* reduction_weight, int B,
                                int T, float* X_out, float* y_out, int out_on_device);

/* The peak of one resident song, taken on the device from its rows: *peak = np.max([np.abs(X).max(), np.abs(y).max()]) of the song's two
 * arrays, bit for bit (lib/dataset.py:214, the coef of a training row and the normaliser of a validation song).  np.abs of a complex64
 * is, in numpy 1.25 and later on a CPU with fused multiply-add, larger * sqrt(fma(r, r, 1)) with r = smaller / larger in float32 -- not
 * hypotf; the device computes exactly that per element, finds the element of largest value -- ties to the lowest (slab, index), so two
 * calls agree in every output -- and the host forms the float from that one element by the same operations.  at[2] (re, im of that
 * element), *slab (0 = X, 1 = y) and *index (its flat complex index in the slab, (row * 2 + channel) * bins + bin) may each be NULL.
 * A NaN in either array (beside no infinite part of the same element) makes *peak NaN, as np.max does; at, slab and index then
 * describe the largest element that is not NaN.  Runs on the store's own stream and returns when the result is on the host.
 * Errors, VR_ERR_BAD_ARGUMENT before anything is launched: a null d or peak, a song index out of range. */
int vr_dataset_peak(vr_dataset d, int song, float* peak, float* at, int* slab, int64_t* index);

/* Windows of resident songs, the validation patches of lib/dataset.py:220-248 without the patch files: sample b is rows
 * [start, start + T) of song w[b].song.  start may be negative and the window may end past the song, or lie wholly outside it: a row
 * outside [0, rows) reads as zero (np.pad).  Every value read is multiplied by w[b].scale, real and imaginary part each, one float32
 * product -- pass 1 / peak as a float32, which is what numpy's complex64 / float32 computes.  Outputs as vr_dataset_batch: X_mag, y_mag
 * [B][2][bins][T] fp32 hypotf of the scaled values; the _complex entry stores the scaled complex64 values themselves.  Runs on the
 * handle's stream and returns when the outputs are complete.
 * Errors, all VR_ERR_BAD_ARGUMENT and all before anything is launched: B <= 0 or a null table (reported before the handle and the store
 * are looked at); a handle on another device than the store; T <= 0; and, with vr_last_error() naming the sample: a song index out of
 * range, start + T overflowing an int64, a scale that is not finite. */
typedef struct vr_window { int song; int reserved; int64_t start; float scale; } vr_window;
int vr_dataset_windows(vr_handle h, vr_dataset d, const vr_window* w, int B, int T, float* X_mag, float* y_mag, int out_on_device);
int vr_dataset_windows_complex(vr_handle h, vr_dataset d, const vr_window* w, int B, int T, float* X_out, float* y_out, int out_on_device);

/* The WAVE store, a second kind of vr_dataset: a song is kept as its two ALIGNED WAVES instead of their STFT rows --
 * half the device bytes as float32 (hop * 4 bytes against bins * 8 per hop and channel), a quarter as the file's PCM16 frames, and no cache
 * file to write or read -- and every entry point above forms the rows it needs on the device: rows [start, start + T) of a song's
 * spectrogram depend on its samples alone, and the crop-table form of the frame-tiled STFT writes them bit for bit as vr_pair_rows_many
 * writes them for the whole wave (row 0 reaches n_fft / 2 zeros in front of the wave, the last rows reach past its end).  The kind of a
 * store is fixed at creation: vr_dataset_add on a wave store and the two calls below on a rows store are VR_ERR_BAD_ARGUMENT.
 *   vr_dataset_create_waves   an empty wave store with its own FFT plan (window and twiddles as every handle builds them); bins =
 *                       n_fft / 2 + 1.  hop_length != n_fft / 2, or an n_fft the frame-tiled kernels do not take (a power of two from 128
 *                       up to what the tile holds in LDS): VR_ERR_UNSUPPORTED, judged on the host before the device is touched.
 *   vr_dataset_add_waves      one song: mix, inst float32 [2][n], already aligned, both on the host or both on the device; each is copied
 *                       once into one device slab (host memory through the store's bounded pinned staging).  vr_dataset_rows reports
 *                       1 + n / hop_length.  OOM as vr_dataset_add.
 *   vr_dataset_add_pcm        the same song as `frames` interleaved frames of 1 or 2 channels (one channel is up-mixed) in a vr_pcm_format,
 *                       channel count and format per wave.  The bytes are stored as they are and decoded where the STFT reads them
 *                       (csrc/pcm.h): every batch, window and peak equals, bit for bit, that of the song added as its decoded floats
 *                       (vr_pcm_convert_host).  The buffers may lie at any byte, host or device.
 *   vr_dataset_info counts the bytes of the slabs (sample bytes rounded up to whole 32-bit words).
 * vr_dataset_batch[_complex], vr_dataset_windows[_complex] and vr_dataset_peak keep their signatures, checks and results: on a wave store
 * a batch is two launches -- the crop STFT of B * (2..4) signals of T rows into scratch of the calling handle (its input-pipeline buffer,
 * reserved for 4 * B signals whatever the flags, so its size follows from B and T alone: 4 * B * T * 2 * bins * 8 bytes plus one
 * eighth, grown once and kept -- vr_pipeline_buffer reports and releases it; two handles never share it), then the augmentation kernel of the rows store
 * reading that scratch; windows transform only the rows inside the song (a row outside is zero, not the transform of padded samples); the
 * peak passes the song's rows through scratch of the store's own, 1024 rows at a time, and merges the chunk candidates by the kernel's
 * rule, so peak, at, slab and index are those of a rows store holding the vr_pair_rows_many rows of the same waves, NaN cases included.
 * One more check, before anything is launched: the handle's n_fft and hop_length must be the store's, else VR_ERR_BAD_ARGUMENT naming
 * both; and B <= 16383.  No float atomics: two identical calls agree bit for bit. */
int vr_dataset_create_waves(int device, int n_fft, int hop_length, vr_dataset* out);
int vr_dataset_add_waves(vr_dataset d, const float* mix, const float* inst, int on_device, int64_t n, int* song_out);
int vr_dataset_add_pcm(vr_dataset d, const void* mix_bytes, const void* inst_bytes, int on_device, int64_t frames, int mix_channels,
                       int inst_channels, int mix_fmt, int inst_fmt, int* song_out);

/* torch.optim.Adam(lr, betas=(b1,b2), eps, weight_decay=0).step()   train.py:215-218,95
 * grad_scale multiplies every gradient first (1/world_size after a SUM all-reduce).  Hyper-parameters are doubles
 * like torch's python floats: 1 - beta, the bias corrections and lr / bias_correction1 are formed in double and only
 * then rounded to the fp32 the parameters live in (1 - 0.999f differs from 0.001f by 1.3e-5 relative).          */
int vr_adam_step(vr_handle h, double lr, double b1, double b2, double eps, double grad_scale);
int vr_zero_grad(vr_handle h);                                          /* model.zero_grad(), train.py:96 */
/* optimizer.state_dict() / load_state_dict() for a resumable checkpoint (the reference saves the model only,
 * train.py:290): the Adam moments as flat host arrays of vr_grad_arena's element count (arena order) + the step. */
int vr_get_adam_state(vr_handle h, float* exp_avg, float* exp_avg_sq, int64_t numel, int64_t* step);
int vr_set_adam_state(vr_handle h, const float* exp_avg, const float* exp_avg_sq, int64_t numel, int64_t step);
int vr_get_grad(vr_handle h, const char* key, float* host, int64_t capacity_bytes);   /* param.grad, torch layout */
/* nn.Dropout2d(0.1) on the five ASPP outputs (lib/layers.py:90), live in train mode.  mode 1 (the DEFAULT, as in
 * the reference): device-side counter-based generator keyed on (seed, number of train-mode forwards so far), a
 * fresh draw per forward; 0: off (explicit opt-out, parity tests);
 * 2: injected keep-masks [5][B][8*nout] holding 0 or 1/0.9 (parity tests), nets in the order
 * stg1_low, stg1_high, stg2_low, stg2_high, stg3_full, row pitch 8*c of each net.                   */
int vr_set_dropout(vr_handle h, int mode, uint64_t seed, const float* masks, int B);
/* The single flat fp32 gradient bucket (device pointer + element count) for the data-parallel
 * all-reduce: vr_allreduce_grads sums it in place with the library's own RCCL communicator (or a caller may reduce this view
 * through torch.distributed -- Trainer(backend='torch' | 'staged')), then vr_adam_step.                                      */
int vr_grad_arena(vr_handle h, float** device_ptr, int64_t* numel);

/* One batch of train.validate_epoch (train.py:117-127), eval mode:
 *   y_pred = model.predict(X); y = spec_utils.crop_center(y, y_pred); loss = nn.L1Loss()(y_pred, y)
 * X, y: [B, 2, bins, T] fp32 (a VR_CREATE_COMPLEX handle with "complex_train" on: complex64, the loss on the complex difference).  *loss_out = loss.item().  Forward, crop and the L1 reduction run on the device. */
int vr_validate_step(vr_handle h, const float* X, const float* y, int on_device, int B, int T, float* loss_out);

/* ---- data-parallel exchange.  The reference has none: train.py:211-213 takes one --gpu. ----
 * One process per GPU, one handle per process.  Rank 0 draws an id (vr_comm_unique_id, 128 bytes = ncclUniqueId),
 * hands it to the other ranks by any host channel (INTEGRATION.md uses torch.distributed's store), every rank calls
 * vr_comm_init.  Per optimizer step: vr_train_step -> vr_allreduce_grads -> vr_adam_step(grad_scale = 1/world).
 * Parity definition: N ranks == the reference's gradient accumulation with accumulation_steps = N (train.py:91-96).
 * RCCL is dlopen()ed on first use (the copy already mapped in the process, e.g. torch's, else the system's).      */
#define VR_COMM_ID_BYTES 128
int vr_comm_unique_id(void* id_out);
int vr_comm_init(vr_handle h, int rank, int world_size, const void* id);
int vr_comm_destroy(vr_handle h);
/* In-place SUM all-reduce of the flat gradient arena (vr_grad_arena) over RCCL/xGMI, enqueued on the handle's stream
 * (no host synchronisation; vr_adam_step follows on the same stream).  wire_dtype 0: fp32 bucket; 1: bf16 bucket
 * (rounded to bf16, summed in bf16 on the wire, widened back to the fp32 arena: half the bytes per link).         */
int vr_allreduce_grads(vr_handle h, int wire_dtype);
/* Rank `root`'s parameters, BatchNorm buffers and num_batches_tracked (and, with_optimizer != 0, the Adam moments and
 * step count) replace every rank's: replicas start identical (what DistributedDataParallel does at construction). */
int vr_broadcast_params(vr_handle h, int root, int with_optimizer);

/* ---- audio front end (no model handle, `device` = GPU index, host pointers) ----------------
 * vr_resample: the resampling step of librosa.load(path, sr=sr_out, res_type='kaiser_fast')   inference.py:136-138,
 * lib/spec_utils.py:139-142.  x [channels][n_in] at sr_in -> y [channels][n_out], n_out = ceil(n_in * sr_out / sr_in)
 * (librosa's fix_length: resampy yields int(n_in * ratio) samples, the rest is zero).  resampy~=0.4 is a third-party
 * dependency of the reference that is not vendored: its published 'kaiser_fast' filter is restated (parity unpinned).
 * vr_xcorr_argmax: np.argmax(np.correlate(a, b, 'full'))        lib/spec_utils.py:107-108 (align_wave_head_and_tail). */
int vr_resample(int device, const float* x, int channels, int64_t n_in, int sr_in, int sr_out, float* y, int64_t n_out);
int vr_xcorr_argmax(int device, const float* a, int64_t na, const float* b, int64_t nb, int64_t* argmax_out);

/* ---- the streamed resampler: vr_resample on blocks, with bounded state ----------------------------------------------
 * A session takes audio x [channels][n] at sr_in in pushes of any sizes >= 1 followed by one flush.  CONTRACT: the concatenation of
 * everything it returned IS what vr_resample returns for the whole input -- bit for bit, the same length ceil(n_in * sr_out / sr_in),
 * the same zero samples behind resampy's int(n_in * ratio) -- however the input was split.  It is exact because output sample t of the
 * kernel depends on t alone, reads at most K = 8193 / index_step inputs on either side of n(t) = floor(t / ratio) and sums them in a
 * fixed order: the session runs the same kernel source on global t and n.  A sample is FINAL, and returned, once input n(t) + K has
 * arrived (from then on the right-hand clamp n_in - n - 1 is inactive whatever n_in turns out to be); the flush computes the rest with
 * the clamp active and appends the zero tail.
 * vr_resampler_push returns every sample that is final: *n_out per channel, possibly 0, at y [channels][capacity] (channel pitch =
 * capacity).  A capacity below what the call returns is VR_ERR_BAD_ARGUMENT, reported before anything is consumed; vr_last_error()
 * names the size needed (vr_resampler_plan computes it: samples_out after minus before).  x, y: host or device pointers, as flagged.
 * vr_resampler_flush ends the session.  sr_in == sr_out is a pass-through session: it returns its input, on the same schedule as any
 * other pair (K = 16), so that a caller's capacity arithmetic has no special case.
 * vr_resampler_push_many: session k receives n_in[k] >= 0 samples and, where flush[k] != 0, its input ends there (flush == NULL: none
 * ends); n_in[k] == 0 without flush leaves session k untouched.  ONE kernel launch serves all sessions -- the launch table carries each
 * session's ratio and filter table, so the sessions may have different rate pairs -- and session k returns exactly what
 * vr_resampler_push (then vr_resampler_flush) on it alone would return.
 * vr_resampler_info: lookahead_samples = K + 1, the input that must have arrived before the first output sample; state_bytes = what a
 * session carries from push to push: the last 2K + 2 input samples per channel, the filter table and its differences (2 x 8193
 * doubles, computed once at open), two 64-bit counters.  It depends on (channels, sr_in, sr_out) and not on how much audio has passed.
 * Besides that a session holds staging for one push: two window buffers of history + the largest push seen (used in turn) and, for
 * host destinations, one output buffer; they grow when a larger push arrives and are otherwise reused.  A session owns its HIP stream
 * and its device memory; every call returns when its outputs are complete.
 * vr_resampler_plan (host only, no session, no GPU) is the schedule the executor follows, from the very expressions of vr_resample:
 * ratio = (double)sr_out / sr_in; n(t) = (long long)((double)t * (1.0 / ratio)); samples_out = the number of t with n(t) + K <
 * samples_in, or, flushed, ceil(samples_in * ratio).
 * Errors (VR_ERR_BAD_ARGUMENT, before the device is touched): non-positive rates or channels, more than 65535 channels or sessions
 * in one call, sr_out / sr_in below 1 / 512, n < 0,
 * push or flush after a flush, a flush with no sample received (vr_resample refuses n_in <= 0 too); in vr_resampler_push_many also a
 * session listed twice, sessions on different devices or with different channel counts, vr_last_error() starting "resampler <k>: ".
 * A call that fails half way (a HIP error) leaves its sessions unusable: close them. */
typedef struct vr_resampler_s* vr_resampler;
int vr_resampler_open(int device, int channels, int sr_in, int sr_out, vr_resampler* out);
int vr_resampler_push(vr_resampler r, const float* x, int x_on_device, int64_t n, float* y, int y_on_device, int64_t capacity,
                      int64_t* n_out);
int vr_resampler_flush(vr_resampler r, float* y, int y_on_device, int64_t capacity, int64_t* n_out);
int vr_resampler_push_many(int n, const vr_resampler* r, const float* const* x, int on_device, const int64_t* n_in, const int* flush,
                           float* const* y, int y_on_device, const int64_t* capacity, int64_t* n_out);
/* The file's sample bytes into a session: vr_resampler_push / vr_resampler_push_many with `bytes` = `frames` interleaved frames in format
 * `fmt` (vr_pcm_format) in place of the planar float block.  A block's frames hold the session's channel count, or 1: every session
 * channel then reads the one sample (the up-mix of a mono file).  The resampling kernel reads the float history of the session's window
 * and, behind it, the bytes; the samples the session carries on reach its other window buffer decoded -- the float part by a device
 * copy, the rest stored by the launch itself, which therefore also happens for a push that returns nothing.  Pass-through sessions
 * (sr_in == sr_out) take bytes too and return the decoded samples on the usual schedule.  CONTRACT: each call returns exactly what the
 * float entry point returns for vr_pcm_convert_host of the same bytes (mono repeated per channel) -- samples, n_out and the state left
 * behind, bit for bit; a session may mix float and PCM pushes freely, vr_resampler_flush serves both, vr_resampler_info reports the
 * same state_bytes.  One launch still serves all sessions of vr_resampler_push_many_pcm: rate pair, format and channel count per entry.
 * Host bytes are staged as bytes in a per-session buffer, rounded up to whole 32-bit words.
 * VR_ERR_BAD_ARGUMENT, before the device or any session is touched (many: vr_last_error() starts "resampler <k>: "): an unknown fmt,
 * channels neither 1 nor the session's, frames < 0, bytes NULL with frames > 0, a DEVICE buffer of VR_PCM_S16 / S32 / F32 off its
 * natural alignment, and everything the float forms refuse. */
int vr_resampler_push_pcm(vr_resampler r, const void* bytes, int on_device, int64_t frames, int channels, int fmt, float* y, int y_on_device,
                          int64_t capacity, int64_t* n_out);
int vr_resampler_push_many_pcm(int n, const vr_resampler* r, const void* const* bytes, int on_device, const int64_t* frames,
                               const int* channels, const int* fmt, const int* flush, float* const* y, int y_on_device,
                               const int64_t* capacity, int64_t* n_out);
int vr_resampler_info(vr_resampler r, int64_t* lookahead_samples, int64_t* state_bytes);
int vr_resampler_close(vr_resampler r);
int vr_resampler_plan(int sr_in, int sr_out, int64_t samples_in, int flushed, int64_t* samples_out);

/* ---- measurement hooks (bench.py) ----------------------------------------------------------- */
/* Bracket subsequent calls: every kernel launch is timed with HIP events on the stream it is launched on (the executor runs
 * every kernel on ONE stream while profiling); conv_* aggregate the convolution launches.
 * conv_flops = 2 x multiply-adds of the direct convolutions (the Winograd kernel performs fewer),
 * conv_bytes = algorithmic HBM bytes (virtual input + weights + output of each launch, once each). */
int vr_profile_begin(vr_handle h);
int vr_profile_end(vr_handle h, double* conv_ms, double* conv_flops, int* conv_launches, double* conv_bytes);
/* Per-kernel totals of the step bracketed by the last vr_profile_begin / vr_profile_end: EVERY kernel the library launched
 * (HIP events on the stream each launch went to), one text line per kernel name
 *     name \t calls \t milliseconds \t algorithmic FLOPs \t algorithmic HBM bytes \t calls that carried figures \n
 * (FLOPs / bytes: convolutions = 2 x multiply-adds of the direct form and input + output + weights once each -- forward,
 * data-gradient and weight-gradient launches alike; element-wise kernels = bytes read + written once; 0 where a kernel has no
 * noted figure).  Returns the size needed incl. the terminator; copies at most `capacity` bytes.  bench.py builds
 * `roofline.classes` from it. */
int64_t vr_profile_report(vr_handle h, char* buf, int64_t capacity);

/* ---- test hooks (tests/ only) ---------------------------------------------------------------- */
/* One convolution through the library's conv dispatcher: x [N,Cin,H,W], w OIHW, padding = dilation
 * (3x3) or 0 (1x1).  `upsample` is a flag word: bit 0 = fused bilinear x2 upsample of x; bit 1 = also
 * hand the launch Winograd-domain weights (3x3 stride-1 only; taken when the input is plain and
 * stats_out is null); bit 2 = `affine`/`slope` are the EPILOGUE ([Cout][2] folded BatchNorm +
 * activation, the eval-mode form) instead of a pending affine [Cin][2] on the input.
 * stats_out [Cout][2] receives (sum, sumsq) of the raw output per channel when non-null.          */
int vr_debug_conv2d(vr_handle h, const float* x, int N, int Cin, int H, int W, const float* w, int Cout,
                    int ksize, int stride, int dil_h, int dil_w, int upsample, const float* affine,
                    float slope, const float* bias, float* out, float* stats_out);
/* Backward of the same single convolution through the MFMA data-gradient / weight-gradient kernels:
 * dz [N,Cout,Hout,Wout] -> dx_out [N,Cin,H,W] (gradient w.r.t. the activated, pre-upsample input
 * values) and dw_out (OIHW).                                                                       */
int vr_debug_conv2d_backward(vr_handle h, const float* x, int N, int Cin, int H, int W, const float* w, int Cout,
                             int ksize, int stride, int dil_h, int dil_w, int upsample, const float* affine,
                             float slope, const float* dz, float* dx_out, float* dw_out);
/* Host half of --postprocess (no GPU involved): per-frame mask minimum [T] -> merge_artifacts blend
 * weight [T] (lib/spec_utils.py:64-87), incl. the reference's IndexError / ValueError cases.        */
int vr_debug_merge_artifacts_weight(const float* frame_min, int T, float thres, int min_range, int fade_size,
                                    float* weight_out);
/* The same weights from the incremental form a VR_STREAM_POSTPROCESS stream runs (csrc/stream_post.h, the code the device walk runs; the
 * constants are fixed: 0.05 / 64 / 32), no GPU involved.  The minima are taken in steps: step k ends in front of frame cuts[k]
 * (0 < cuts[0] <= cuts[1] <= ... <= T), one more step takes the rest, then the flush.  The weights live in a ring of 161 + (the largest
 * step) entries; a frame is copied to weight_out at the moment it is declared final: after a step that ends in front of frame h the
 * frames below h - 161, at the flush all.  final_after_out [n_cuts + 1] (may be NULL): the frames declared final after each of the
 * n_cuts steps, then T.  All minima at or below the threshold give zeros, no error. */
int vr_debug_stream_post_weight(const float* frame_min, int T, const int* cuts, int n_cuts, float* weight_out, int* final_after_out);
/* One kernel of the training path or of the signal front end in isolation, host pointers in and out (csrc/debug.hip lists
 * the names, their dims / float parameters / inputs / outputs): bn_backward, lstm, upsample, pool, thin, head_loss, rows,
 * adam, wire, signal_norm, signal_mask, wave_eval, stream_post.                                                        */
int vr_debug_kernel(vr_handle h, const char* name, const int64_t* dims, int ndims, const float* fparams, int nfparams,
                    const float* const* inputs, int ninputs, float* const* outputs, int noutputs);
/* Record intermediate activations of the next vr_forward and read them back (post-activation). */
int vr_debug_record_taps(vr_handle h, int enable);
int64_t vr_debug_get_tap(vr_handle h, const char* name, float* host, int64_t capacity_floats, int64_t* shape4);

#ifdef __cplusplus
}
#endif
#endif /* VR_MI355_H */
