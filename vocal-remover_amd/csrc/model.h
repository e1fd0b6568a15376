// Host-side model: parameter registry (reference state_dict keys), network topology of
// lib/nets.py / lib/layers.py, forward executor, and the device-resident Separator pipeline.
#pragma once
#include <chrono>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"
#include "weight_forms.h"

namespace vr {

// Bump allocator over one device slab; `dry` mode only measures.
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    bool dry = false;
    void* alloc(size_t bytes) {
        const size_t a = (off + 255) & ~size_t(255);
        off = a + bytes;
        if (off > peak) peak = off;
        if (dry) return reinterpret_cast<void*>(uintptr_t(256));   // non-null dummy, never dereferenced
        if (off > cap) throw Error(-4, "workspace arena overflow (planning bug)");
        return base + a;
    }
    float* allocf(size_t n) { return static_cast<float*>(alloc(n * sizeof(float))); }
    void reset() { off = 0; }
};

enum ParamKind { PK_PLAIN = 0, PK_CONV = 1, PK_LSTM_IH = 2, PK_BUFFER = 3, PK_NBT = 4 };

struct Param {
    std::string key;
    std::vector<int64_t> shape;     // torch shape
    ParamKind kind = PK_PLAIN;
    size_t numel = 0;               // torch numel
    size_t dev_numel = 0;           // device footprint (floats) incl. padding
    size_t off = 0;                 // offset (floats) into its arena
    bool trainable = true;
    // PK_CONV / PK_LSTM_IH layout info: device layout [Cin][KK][CoutPad]
    int Cout = 0, Cin = 0, KK = 1, CoutPad = 0, co_off = 0;
    Param* alias_of = nullptr;      // PK_LSTM_IH reverse half lives inside the forward half's buffer
    float* dev = nullptr;
    int64_t nbt = 0;                // PK_NBT value (host)
    float* grad_override = nullptr; // test hook: gradient slot outside the arena
};

struct BN {
    int C = 0;
    Param *w = nullptr, *b = nullptr, *rm = nullptr, *rv = nullptr, *nbt = nullptr;
    float* affine = nullptr;        // [rows][2] scale, shift (device)
    int bcast = 0;                  // >0: C==1, affine replicated to this many rows
    float* save_mean = nullptr;
    float* save_invstd = nullptr;
};

struct Conv {
    std::string name;
    int Cin = 0, Cout = 0, CoutPad = 0, KS = 3, stride = 1, dh = 1, dw = 1, pad_h = 1, pad_w = 1;
    Param* w = nullptr;
    BN* bn = nullptr;
    float slope = 0.f;              // activation after the BatchNorm
    FormClass cls = FC_NONE;        // which derived weight forms the layer's shape asks for (weight_forms.h)
    WeightForms forms;              // ... and the ones it holds
};
inline FormSpec form_spec(FormId f, const Conv& L, int mfma_mode, Wino6Want w6) {
    return form_spec(f, L.cls, L.Cin, L.Cout, L.KS * L.KS, L.CoutPad, mfma_mode, w6);
}

struct LSTMMod {
    Conv squeeze;                   // 1x1 conv 2c -> 1 (+BN+ReLU), run by the thin-conv kernel
    int nin = 0, hid = 0;           // LSTM input size (= nbins at dec2 level), hidden per direction
    Conv proj;                      // W_ih of both directions as one 1x1 conv (nin -> 8*hid), no BN
    Param *b_ih_f = nullptr, *b_hh_f = nullptr, *b_ih_r = nullptr, *b_hh_r = nullptr;   // [4H] each
    Param *whh_f = nullptr, *whh_r = nullptr;
    Conv dense;                     // Linear(2*hid -> nin) as 1x1 conv + BatchNorm1d + ReLU
    Param* dense_b = nullptr;
    float* bias_sum = nullptr;      // eval: b_ih + b_hh of both directions [2][4H], refreshed with the folded affines (saves two launches per LSTM and call)
};

struct BaseNetL {
    std::string prefix;
    int c = 0;
    Conv enc1;
    Conv enc_a[4], enc_b[4];        // enc2..enc5: conv1 (stride 2), conv2
    Conv aspp_pool, aspp_c2, aspp_d[3], aspp_bott;
    float* aspp_aff = nullptr;      // [4*8c][2]: affine tables of conv2..conv5 laid out contiguously
    Conv dec[4];                    // dec4, dec3, dec2, dec1
    LSTMMod lstm;
};

void comm_unique_id(void* out128);                       // ncclGetUniqueId (comm.hip)

// host half of spec_utils.merge_artifacts (lib/spec_utils.py:60-93): per-frame mask minimum -> blend weight
void merge_artifacts_weight(const std::vector<float>& fmin, std::vector<float>& weight, float thres, int min_range,
                            int fade);


// The schedule of a streaming session (vr_stream_plan: the one statement of it, the executor follows it).  hop == n_fft / 2: frame t
// reads the samples [(t-1) hop, (t+1) hop), so it is ready once (t+1) hop samples have arrived, or -- zeros behind the data -- at flush,
// when the frame count becomes the offline 1 + L / hop.  Crop i of pass 0 covers the frames [i roi - offset, (i+1) roi + offset) and
// gives the mask of [i roi, (i+1) roi); pass 1 (tta) is the same list shifted by -roi/2.  A crop runs once every frame of its window
// is ready, at flush the offline count of make_padding.  Frame t is final when the crops of both passes that hold its mask have run;
// with `out_done` frames out, hop * (out_done - 1) output samples are final.  out_done = done, or for a --postprocess stream (DESIGN.md
// section 6w) the frames whose merge_artifacts weight is final too: every frame once flushed, else done - kStreamPostDelay (0 below 2: a
// lone first frame gives no sample).
struct StreamSchedule { long long frames, crops[2], done, samples_out, out_done; };
StreamSchedule stream_schedule(int n_fft, int hop, int cropsize, int offset, int tta, long long samples_in, int flushed, int postprocess = 0);

// Evaluation against the true stems (vr_evaluate_wave*): what Model::separate_run needs beyond a wave-level call.
// inst[s]: song s's true instruments [2][L[s]], where the mixtures are (host or device); sums[s]: HOST [windows][4] doubles;
// stems false: the call returns sums only (y, v of separate_run unused).
struct EvalArgs { const float* const* inst; long long window; double* const* sums; bool stems; };
// Pseudo-instrument labels (vr_pseudo*): the input of song s is the pair (in[s], inst[s]) -- two spectrograms or two
// waves of the same size, where the mixtures are (host or device); the network separates D = in - inst, and y[s] receives
// P = inst + instruments stem of D, T complex64 frames in `layout` (enum vr_pseudo_layout).  v of separate_run is unused.
struct PseudoArgs { const float* const* inst; int layout; };
// Spectrogram images of the stems (vr_separate_*_img): y_img[s] / v_img[s] receive song s's pictures [bins][T][3]
// bytes, where the stems go (host or device); ranges (HOST, may be null) [song][stem][2] = (lo, max - lo) of each picture.  stems false:
// pictures only (y, v of separate_run unused).
struct ImageArgs { uint8_t* const* y_img; uint8_t* const* v_img; float* ranges; bool stems; };
// the stems' length and the window count of a song of L samples: samples = hop (L / hop), windows = ceil(samples / window); host only
struct EvalPlan { long long samples, windows; };
EvalPlan evaluate_plan(int hop, long long L, long long window);

// One streaming session of a handle (vr_stream_*): everything that outlives a push.  Device state is one slab whose size depends on
// (n_fft, cropsize, batchsize, tta, postprocess) only.
struct StreamState {
    int cropsize = 0, bs = 0, roi = 0, R = 0, RM = 0, chunk_frames = 0;
    bool tta = false, measure = false, running = false, pcm16 = false, post = false;
    bool flushed = false, broken = false;
    long long samples = 0, tail_base = 0;
    long long frames = 0, crops[2] = {0, 0}, done = 0;   // done: frames whose mask is final
    long long out_done = 0;                              // frames given out (= done unless post)
    char* slab = nullptr; size_t state_bytes = 0;
    float* tail[2] = {nullptr, nullptr}; int tail_cur = 0;
    float2* ring = nullptr;
    float* mask[2] = {nullptr, nullptr};
    float* carry[2] = {nullptr, nullptr}; int carry_cur = 0;
    unsigned* stats = nullptr;                           // launch_mag_pad's layout: 16-byte header + 2 * bins rows of partial maxima
    float* aff = nullptr;                                // 1 / c as the crop gather reads it
    // post: per-frame mask minima and merge_artifacts weights, frame t at [t % RW], and the state of the walk (stream_post.h)
    int RW = 0;
    float* fmin_ring = nullptr;
    float* wgt_ring = nullptr;
    StreamPostState* post_state = nullptr;
    double coef[2] = {0.0, 0.0};                         // MEASURE: the normaliser, valid after flush
};

// The resident training set (vr_dataset_*): every song's cached spectrogram pair copied once into two device slabs of
// [rows][2][bins] complex64, the on-disk layout of spec_utils.SpectrogramCache.  The store owns its allocations and nothing of any
// handle: it may outlive handles, and every handle on its device may cut batches from it (Model::dataset_batch_api).
struct ResidentCrop { int song, mix_song; long long start, mix_start; };        // layout-compatible with vr_crop
struct ResidentWindow { int song, reserved; long long start; float scale; };    // layout-compatible with vr_window
struct PeakCand;
// A second kind, fixed at creation, the WAVE store: a song is its two aligned waves -- planar float32 [2][n], or
// the file's interleaved sample bytes as they are -- in one slab each (X, y then point to those), rows = 1 + n / hop, and every entry
// point forms the rows it needs with the crop-table form of the frame-tiled STFT (launch_stft_crops) from the store's own FFT plan.
struct ResidentSet {
    struct Song {
        float2* X; float2* y; long long rows;
        long long n = 0;                                                        // (wave store) samples per channel
        int fmt[2] = {0, 0}, channels[2] = {2, 2};                              // (wave store) per slab: 0 = planar float32, else vr_pcm_format
    };
    int device, bins;
    std::vector<Song> songs;
    long long bytes = 0;
    bool waves = false;                                                         // the store kind
    int n_fft = 0, hop = 0;                                                     // (wave store)
    FFTPlan plan{};                                                             // (wave store) window and twiddles from fft_plan_create
    ResidentSet(int device, int bins);
    ResidentSet(int device, int n_fft, int hop);                                // the wave store
    // (wave store) one song from two float waves [2][n], host or device / from two blocks of interleaved sample bytes -> song index
    int add_waves(const float* mix, const float* inst, bool on_dev, long long n);
    int add_pcm(const void* mix, const void* inst, bool on_dev, long long frames, const int* channels, const int* fmt);
    // one CropSeg for rows [start, start + T) of slab `which` (0 = mixture, 1 = instrumental) of a song of the wave store
    CropSeg crop_seg(int song, int which, long long start, int T, float2* dst) const;
    ~ResidentSet();
    ResidentSet(const ResidentSet&) = delete;
    ResidentSet& operator=(const ResidentSet&) = delete;
    int add(const float* X, const float* y, long long rows);                    // -> song index
    // vr_dataset_peak: np.max([np.abs(X).max(), np.abs(y).max()]) of one song, on the store's own stream; returns with the result
    float peak(int song, float* at, int* slab, long long* index);
private:
    PeakCand* peak_ws = nullptr;                                                // kPeakParts + 1 candidates (kernels.h), made at the first peak
    static constexpr size_t kPiece = size_t(8) << 20;                           // upload staging: two pinned pieces, never a whole song
    hipStream_t up = nullptr;
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t drained[2] = {nullptr, nullptr};
    void upload(float2* dst, const float* src, size_t n_bytes);
    int add_slabs(const void* const src[2], const size_t slab[2], bool on_dev, const Song& proto, const char* who);
    // (wave store) vr_dataset_peak's bounded scratch: kPeakChunkRows rows of both slabs and a table of two entries, made at the first peak
    static constexpr int kPeakChunkRows = 1024;
    char* peak_rows = nullptr;
    float peak_waves(int song, float* at, int* slab, long long* index);
};

// ---- the train-form head (train.hip): mask head -> loss -> dmask -> dlogit -> thin weight and data gradients of one feature tensor f3
// [N][C][H][W], in its four forms: real L1, complex L1 (kind 0), VR_LOSS_MAG_L1_WAVE_SDR (1) and VR_LOSS_MAG_L1_WAVE_WSDR (3), the last
// two on complex heads.  The fused train step, the split step's backward and the head_* hooks of debug.hip all run this one function.
struct HeadScratch {
    float *dlogit, *lpart, *wpart;                       // [N][CO][H][W], head_loss_blocks(f3), thin_wgrad_blocks(f3) * CO * C
    float *mask, *dmask, *wave[3], *part, *table;        // kinds 1 / 3: complex64 [N][2][bins][W] each, the y, p (kind 3: and x) waves,
};                                                       // the wave term's partials and table slot (wave_term_floats)
struct TrainHead {
    int kind; bool cplx;
    const float *w, *X, *Y; int bins;                    // the head weights [CO][C]; X, Y [N][2][bins][W] (cplx: complex64)
    float* mask;                                         // null: kind 0 writes no mask, kinds 1 / 3 keep it in the scratch
    float* loss;                                         // [1], [4] or [7]: the loss or its magnitude term, then the three or six wave sums
    float loss_scale, grad_scale, sdr_scale;             // 1 / ntot, 1 / (ntot accumulation_steps), sdr_weight / accumulation_steps
    float* g; int g_acc; float* dw; int dw_acc;          // dL/df3 and dL/dw, stored (0) or added (1); dw null: the head kernel alone
};                                                       // (mask, loss[0] and, kind 0, dlogit)
// the scratch from `allocf` (floats -> pointer), in one fixed order: a dry run and the real run size alike
template <class ALLOC>
HeadScratch head_scratch(ALLOC&& allocf, const FFTPlan& pl, int hop, const Tensor& f3, int kind, bool cplx, int bins) {
    const int CO = cplx ? 4 : 2;
    HeadScratch s{};
    s.dlogit = allocf((size_t)f3.N * CO * f3.H * f3.W);
    s.lpart = allocf((size_t)head_loss_blocks(f3));
    s.wpart = allocf((size_t)thin_wgrad_blocks(f3) * CO * f3.C);
    if (kind == 0) return s;
    const WaveTermFloats wf = wave_term_floats(pl, hop, kind, f3.N * 2, f3.W);
    s.mask = allocf((size_t)f3.N * 2 * bins * f3.W * 2);
    s.dmask = allocf((size_t)f3.N * 2 * bins * f3.W * 2);
    for (int i = 0; i < wf.waves; ++i) s.wave[i] = allocf(wf.wave);
    s.part = allocf(wf.part);
    s.table = allocf(wf.table);
    return s;
}
void run_train_head(const FFTPlan& pl, const Tensor& f3, const TrainHead& h, const HeadScratch& s, WaveTable* staging, hipStream_t st);
// its tail, for a caller that has dlogit already: the thin weight and data gradients
void launch_head_grads(const Tensor& f3, int CO, const float* w, const float* dlogit, float* wpart, float* g, int g_acc, float* dw,
                       int dw_acc, hipStream_t st);

void fft_plan_create(FFTPlan& plan, int n_fft);           // twiddles and the periodic Hann window of one n_fft, on the current device

class Model {
public:
    Model(int device, int n_fft, int hop, int nout, int nout_lstm, bool is_complex = false);
    ~Model();

    int device, n_fft, hop, nout, nout_lstm, max_bin, output_bin, offset = 64;
    // CascadedNet(is_complex=True) (lib/nets.py:46-141): the input is the complex spectrogram as nin = 4 planar channels
    // [re L, re R, im L, im R], the head predicts a complex mask bounded by tanh(|m|), every mask buffer is complex64.
    // Eval-mode inference only unless complex_train is set: the training entry points refuse such a handle (need_real_mask).
    bool is_complex = false;
    // vr_set_option("complex_train") (default 0, complex handles only): the training entry points take such a handle -- interleaved
    // complex64 X, y, mask, dmask; loss = mean |m X - y| over complex elements.  Off: they refuse it, as before.
    bool complex_train = false;
    // vr_set_loss: 0 = L1 on mask * X - y (the default), 1 = VR_LOSS_MAG_L1_WAVE_SDR, mean | |y| - |mask X| | +
    // sdr_weight * sdr(to_wave(y), to_wave(mask X)); complex_train handles on the tiled signal path only.  vr_train_step and
    // vr_validate_step compute it; last_mag_l1 / last_sdr are the two terms of the last such call (vr_loss_terms).
    int loss_kind = 0;
    double sdr_weight = 0.01, last_mag_l1 = 0.0, last_sdr = 0.0;
    bool loss_terms_valid = false;
    WaveTable wave_host{};                                // the wave term's table entry, staged here for its copy to the device
    // 3 = VR_LOSS_MAG_L1_WAVE_WSDR: the wave term is the reference's weighted_sdr_loss on the target and on the
    // residual; last_sdr is then wsdr and last_y_sdr / last_noise_sdr / last_alpha its three parts (vr_loss_terms_wsdr).
    double last_y_sdr = 0.0, last_noise_sdr = 0.0, last_alpha = 0.0;
    void set_loss(int kind, double weight);
    float finish_wave_loss(const float* l4);
    float finish_wsdr_loss(const float* l7);
    int nin = 2;
    void need_real_mask(const char* what) const;          // refuse a complex handle (training entry points)
    void need_real_mask_train(const char* what) const;    // ... only while it is in training mode

    // ---- parameters ----
    std::deque<Param> params;
    std::map<std::string, Param*> by_key;
    void set_param(const std::string& key, const void* host, const int64_t* shape, int ndim);
    void get_param(const std::string& key, void* host, int64_t cap_bytes);
    void set_training(bool t);
    bool training = false;
    bool fwd_only = false;                               // train-mode vr_forward: batch statistics, no tape, no gradient buffers
    bool taping() const { return training && !fwd_only; }

    // ---- forward over host or device input ----
    // x: [B,2,output_bin,T] fp32 magnitudes (complex handle: complex64, and out complex64 too).  mode 0: forward (full
    // width), 1: predict_mask (offset crop), 2: predict (x*mask, offset crop).  out sized accordingly.
    void forward_api(const float* x, bool x_on_device, int B, int T, int mode, float* out, bool out_on_device);

    // train.validate_epoch body for one batch (train.py:117-127): predict + crop_center(y) + L1, on the device
    void validate_api(const float* X, const float* Y, bool on_dev, int B, int T, float* loss_out);
    // tests only: one kernel of the training path, host pointers (debug.hip)
    void debug_kernel(const std::string& name, const int64_t* dims, int ndims, const float* fp, int nfp,
                      const float* const* in, int nin, float* const* out, int nout);

    void debug_conv_launch(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                           int nout);                     // its "conv_launch" entry
    void debug_conv_tail(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                         int nout);                       // "conv_tail": a conv_x3h launch and the 1x1 stage behind it, fused or as two launches
    void debug_wgrad_launch(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                            int nout);                    // "wgrad_launch": one launch_wgrad in its general form
    void debug_wgrad_reduce(const int64_t* dims, int ndims, const float* const* in, int nin, float* const* out, int nout);   // "wgrad_reduce"
    void debug_dgrad_launch(const int64_t* dims, int ndims, const float* const* in, int nin, float* const* out, int nout);   // "dgrad_launch"
    void debug_tensor_pass(const int64_t* dims, int ndims, const float* fp, int nfp, const float* const* in, int nin, float* const* out,
                           int nout);                     // "tensor_pass": one materialize / upsample2x / avgpool_h on a pending tensor
    void debug_weight_form_launch(const int64_t* dims, int ndims, const float* const* in, int nin, float* const* out, int nout);   // "weight_forms"
    void debug_layer_forms(const int64_t* dims, int ndims, float* const* out, int nout);   // "layer_forms": what the handle holds for one conv
    // ---- signal path ----
    void stft_api(const float* wave, bool on_dev, long long L, float* spec, bool spec_on_dev);
    void istft_api(const float* spec, bool on_dev, int T, float* wave, bool wave_on_dev);
    // The offline executor (vr_separate* and vr_separate*_many): n_songs spectrograms (L null: specs [2,bins,T[s]] -> y / v spectrograms)
    // or waves (L given: [2,L[s]] -> y / v waves [2, hop*(T-1)], the whole inference.py pipeline device resident) in one call; with
    // pcm_fmt the waves are sample bytes and the stems int16 [samples][2].  solo: a one-song entry point's call of one song.
    // eval: the evaluation mode of a float wave-level call (EvalArgs above).  pseudo: the pair call (PseudoArgs above), float inputs.
    void separate_run(int n_songs, const float* const* in, bool in_on_dev, const int* T, const long long* L, int tta, int batchsize,
                      int cropsize, float* const* y, float* const* v, bool out_on_dev, const int* pcm_channels = nullptr,
                      const int* pcm_fmt = nullptr, bool solo = false, const EvalArgs* eval = nullptr,
                      const PseudoArgs* pseudo = nullptr, const ImageArgs* image = nullptr);
    // ---- pitch-shifted waves and training pairs (vr_pitch_*, csrc/pitch.hip) ----
    // spec [signals][bins][T] -> out [signals][bins][ceil(T / rate)], the handle's bins and hop
    void phase_vocoder_api(const float* spec, bool on_dev, int signals, int T, double rate, float* out, bool out_on_dev);
    // vr_istft with librosa's length=: the per-frame kernels whatever the hop, wave [2][length]
    void istft_length_api(const float* spec, bool on_dev, int T, long long length, float* wave, bool wave_on_dev);
    // n items through stft -> phase vocoder -> istft(length) -> resample -> fix_length at shift_n_fft / shift_hop, one after the other in one
    // workspace.  inst null: waves[i] [channels][L[i]] -> out[i] of the same shape.  inst given (channels 2): y' = shift(inst), v' =
    // shift(waves - inst), X' = y' + v'; X_out[i] / y_out[i] = their STFTs at the handle's n_fft / hop in `layout`.
    void pitch_run(int n, const float* const* waves, const float* const* inst, bool on_dev, int channels, const long long* L, int shift_n_fft,
                   int shift_hop, double rate, double ratio, long long max_bytes, float* const* out, float* const* X_out, float* const* y_out,
                   int layout, bool out_on_dev);
    // ---- plain training pairs (vr_pair_rows_many, csrc/prepare.hip) ----
    // rows [T][2][bins] of mix[i][:, a_off : a_off + n] and inst[i][:, b_off : b_off + n] at the handle's n_fft / hop (hop == n_fft / 2 only:
    // -9 elsewhere), T = 1 + n / hop, and peaks[i] = max(|X|.max(), |y|.max()) from the rows just written
    void pair_rows_run(int n, const float* const* mix, const float* const* inst, bool on_dev, const long long* L_mix, const long long* L_inst,
                       const PairWindow* w, long long max_bytes, float* const* X_out, float* const* y_out, bool out_on_dev, float* peaks);
    // ---- WAV sample bytes in, PCM16 out (vr_*_pcm*; csrc/pcm.h): the sample-format forms of the frame-tiled STFT / iSTFT ----
    bool pcm_available() const;                           // the frame-tiled kernels, whose forms these are, exist on this handle
    void check_pcm(const void* bytes, int channels, int fmt, const std::string& who) const;      // availability, format, channels, a device pointer's alignment
    void stft_pcm_api(const void* bytes, bool on_dev, long long L, int channels, int fmt, float* spec, bool spec_on_dev);
    void istft_pcm16_api(const float* spec, bool on_dev, int T, int16_t* out, bool out_on_dev);
    void run_crop_chunks(int patches, int bs, const std::function<void(int, int)>& run_crops);
    // ---- streaming separation (vr_stream_*) ----
    StreamState* stream_open(int cropsize, int batchsize, int flags, double coef_re, double coef_im);
    // n samples more (flush: none, the end of the input); y / v [2][capacity] receive *n_out final samples per channel
    // fmt != 0 (vr_stream_push_pcm): `wave` is n interleaved frames of `channels` samples in that format, read by the stream STFT itself
    void stream_push(StreamState& S, const float* wave, bool on_dev, long long n, bool flush, float* y, float* v, bool out_on_dev,
                     long long capacity, long long* n_out, int channels = 0, int fmt = 0);
    // vr_stream_push_many: stream k gets n[k] more samples and, flush[k], its end; the crops of all streams share device batches
    void stream_push_many(int n_streams, StreamState* const* S, const float* const* wave, bool on_dev, const long long* n, const int* flush,
                          int batchsize, float* const* y, float* const* v, bool out_on_dev, const long long* capacity, long long* n_out,
                          const int* channels = nullptr, const int* fmt = nullptr);      // fmt given (vr_stream_push_many_pcm): wave[k] is bytes
    void stream_close(StreamState* S);
    long long pipeline_buffer(bool release);             // bytes of aug_buf held before the call; release: free it
    void arena_bytes(long long* staging, long long* workspace) const { *staging = (long long)io.cap; *workspace = (long long)ws.cap; }

    // ---- debug / test hooks ----
    void debug_conv(const float* x, int N, int Cin, int H, int W, const float* w_oihw, int Cout, int KS, int stride,
                    int dh, int dw, int up, const float* aff, float slope, const float* bias, float* out,
                    float* stats_out);
    // A hook's local conv and the weight forms made for it, by the handle's own rule, allocator and selection; frees them, also when a
    // launch throws.
    struct LocalConv {
        Conv L;
        Param P;
        FormStore store;
        LocalConv() { L.w = &P; }
        ~LocalConv() { store.release(); }
        LocalConv(const LocalConv&) = delete;
        LocalConv& operator=(const LocalConv&) = delete;
    };
    // The device forms of one layer's weights that `mfma_mode` multiplies with, made from the K-major copy dw_kmajor [Cin][KS*KS][CoutPad]
    // through the single-layer launchers and set in `a` (wino / wino6 / x3w); shared by debug_conv and the conv_launch / conv_tail hooks.
    void debug_weight_forms(const float* dw_kmajor, int Cin, int KS, int stride, int dh, int dw, int CoutPad, int Win, bool transformed,
                            ConvArgs& a, LocalConv& lc);
    bool record_taps = false;
    std::map<std::string, Tensor> taps;
    int64_t get_tap(const std::string& name, float* host, int64_t cap_floats, int64_t* shape4);

    // ---- profiling ----
    bool profiling = false;
    LaunchProfiler* launch_prof = nullptr;               // profile.hip: every VR_LAUNCH of a profiled step, timed on its own stream
    std::string profile_report;                          // per-kernel-name totals of the last profiled step (vr_profile_report)
    void profile_begin();
    void augment_api(const float* Xc, const float* yc, const float* Xi, const float* yi, const void* desc, const float* rw,
                     int B, int T, int bins, bool in_on_dev, float* Xmag, float* ymag, bool out_on_dev, bool out_complex = false,
                     bool ex = false);                 // (ex: desc is a table of AugDescEx, the _ex entry points)
    void wave_store_check(const ResidentSet& set, const char* who, int B) const;
    void dataset_batch_api(const ResidentSet& set, const ResidentCrop* crops, const void* desc, const float* rw, int B, int T,
                           float* Xmag, float* ymag, bool out_on_dev, bool out_complex = false, bool ex = false);
    void dataset_windows_api(const ResidentSet& set, const ResidentWindow* w, int B, int T, float* Xmag, float* ymag, bool out_on_dev,
                             bool out_complex = false);
    char* aug_buf = nullptr; size_t aug_cap = 0;         // staging of the training input pipeline
    void aug_reserve(size_t need);
    bool train_wino = true;                              // vr_set_option("train_winograd"): Winograd kernels in train mode
    // vr_set_option("mfma_mode"): how the 3x3 stride-1 convs multiply.
    //   2 (round-3 default) = fp32 products as six bf16 products of three-way split operands on v_mfma_f32_32x32x16_bf16, fp32 accumulation
    //       (conv_x3.hip: direct conv, error vs fp64 = an fp32 direct convolution's; forward and data-gradient convs -- weight
    //       gradients stay on the fp32 MFMA);
    //   0 = v_mfma_f32_32x32x2_f32 throughout (Winograd F(2x2,3x3) / direct kernels, round-1/2 default);
    //   1 = operands rounded to bf16 (configs[4] arithmetic; "mfma_bf16" 1 is the same);
    //   3 (default since round 4) = the layers of mode 2 with fp32-grade products from THREE fp16 products of two-way split,
    //       power-of-two scaled operands on v_mfma_f32_32x32x16_f16 (conv_x3h.hip: 14 instead of 27 matrix instructions per 8-channel
    //       chunk; measured error vs fp64 at or below mode 2's).
    int mfma_mode = 3;
    bool x3_mode() const { return mfma_mode == 2 || mfma_mode == 3; }
    int default_mfma_mode = 3;                           // (VR_MFMA_MODE overrides; "mfma_mode" -1 / "mfma_bf16" 0 return to it)
    bool serial = false;                                 // vr_set_option("serial_exec"): no lanes / side streams (tests: race detector)
    // vr_set_option("crop_window") (default 1): eval, mfma_mode 3, no taps -- a caller that keeps only the columns [w_lo, w_hi) of
    // the mask (predict_mask's offset crop, lib/nets.py:124-128) has the stage-3 dec1 conv compute only the 32-column tiles meeting
    // them (ConvArgs::w_lo / w_hi) and the head read only those; 0 = every column, as before
    bool crop_window = true;
    // vr_set_option("fuse_tail") (default 1): eval, mfma_mode 3, no taps -- the 1x1 stage tails of the low-band nets and the LSTM squeeze
    // run in the epilogue of the conv_x3h launch whose output they alone read (FusedTail); 0 = two launches each, as before
    bool fuse_tail = true;
    // vr_set_option("lstm_gemm") (default 1): eval -- the LSTM input projection and the Linear behind the LSTM run as rows_gemm.hip launches
    // (16 x 16 output tiles, K split over a workgroup's four waves); 0 = run_conv's one-row 1x1 convs, as before
    bool lstm_gemm = true;
    // vr_set_option("aspp_pool_fused") (default 1): eval, where the four ASPP branch convs go out as one conv_x3d launch -- the pooled
    // branch (mean over H + conv1.1) is a fifth part of that launch; 0 = avgpool_h + a 1x1 conv launch in front of it, as before
    bool aspp_pool_fused = true;
    int net_w_lo = 0, net_w_hi = 0;                      // run_net: the columns of the mask the caller keeps (0, 0: all)
    void set_option(const std::string& name, int value);
    void reset_adam_state();
    void profile_end(double* conv_ms, double* conv_flops, double* conv_bytes, int* launches);

    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;          // eval mode: the high-band chain runs here
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool band_fork_active = false;                       // run_net: the side stream currently carries the high-band chain
    bool gs_clear_pending = false;                       // training: the gs memset runs on lanes[0].main beside the forward
    bool wgrad_on_side = false;                          // training: weight gradients in flight on side_stream
    // eval mode, second lane: the crops of a batch are independent, so separate() runs the two halves
    // of the batch as two concurrent chains (own streams, own workspace); the tail of one chain's
    // kernels and its memory-bound kernels (upsample, LSTM, copies) overlap the other chain's convs.
    struct Lane { hipStream_t main = nullptr, side = nullptr; hipEvent_t fork = nullptr, join = nullptr, start = nullptr, done = nullptr; Arena ws; };
    std::vector<Lane> lanes;                             // the additional lanes (VR_LANES - 1, default 1)
    void swap_lane(int i);

private:
    // arenas
    float* p_arena = nullptr; size_t p_floats = 0;      // trainable parameters (kernel layouts)
    float* b_arena = nullptr; size_t b_floats = 0;      // buffers (running stats), affine tables, saves
    Arena ws;                                            // activations workspace
    Arena io;                                            // persistent I/O staging (spec, mask, waves)
    void ensure_ws(size_t bytes);
    int plan_B = -1, plan_T = -1; bool plan_training = false; size_t plan_peak = 0;    // memo of plan_and_reserve
    void ensure_io(size_t bytes);

    std::deque<BN> bns;
    std::vector<BN*> bn_list;
    struct PendingConv { ConvArgs a; ConvShape shp; double flops, bytes; bool stats; BNFinalizeArgs fin; BN* bn; };
    std::vector<PendingConv>* conv_sink = nullptr;       // set: run_conv hands the launch to its caller instead of launching (ASPP branch group)
    int x3d_mode = 2;                                    // option "conv_x3d": 0 off, 1 single launches, 2 + the ASPP branch group
    int conv_w_lo = 0, conv_w_hi = 0;                    // set: the next run_conv stores only these output columns if conv_x3h takes it
    int x3s_mode = x3s_default();                        // option "conv_x3s": the 3x3 stride-2 layers on the fp16 pipe in eval (conv_x3s.hip, mfma_mode 3); 0: conv_dma.hip
    static int x3s_default() { const char* e = getenv("VR_CONV_X3S"); return (e && atoi(e) == 0) ? 0 : 1; }
    // The derived weight forms (weight_forms.h): every conv's record points into form_store's one allocation per form, made when a
    // refresh first fills the form -- an eval-only handle never holds the data-gradient forms, the bf16 planes of U exist only under
    // mfma_mode 2 with VR_CONV_X3=0.  hold_form / fill_form serve the hooks' local convs too (`single`: the single-layer launchers).
    FormStore form_store;
    void hold_form(FormId f, const std::vector<Conv*>& convs, Wino6Want w6, FormStore& s);
    void fill_form(FormId f, const std::vector<Conv*>& convs, Wino6Want w6, FormStore& s, bool single);
    FormSelect form_select() const { return FormSelect{mfma_mode, training, train_wino, x3d_mode, x3s_mode, dry}; }
    // deferred weight-gradient slab sums of one backward pass (launch_wgrad_reduce_batched, round 6)
    std::vector<WgReduceDesc> wred_host, wred_sent;
    WgReduceDesc* wred_dev = nullptr;
    size_t wred_cap = 0;
    void flush_wgrad_sums();
    // the grid sizes of the batched refresh launches, from their descriptor tables (shared with the weight_forms hook of debug.hip)
    static long long x3_batch_max_elems(const std::vector<X3WDesc>& descs);
    static int x3_batch_max_cout_pad(const std::vector<X3WDesc>& descs);
    static long long wino_batch_max_elems(const std::vector<WinoWDesc>& descs, bool split6);
    static long long s2w_batch_max_elems(const std::vector<S2WDesc>& descs);
    void refresh_forms(bool with_dgrad);
    BNFoldDesc* d_fold = nullptr;
    bool affine_dirty = true;
    void fold_eval_affines();

    BaseNetL nets_[5];
    Conv tail1, tail2;                                   // stg{1,2}_low_band_net.1
    Param *out_w = nullptr, *aux_out_w = nullptr;

    FFTPlan plan{};
    FFTPlan shift_plan{};                                // the pitch shifter's transform when it is not the handle's own (pitch.hip)

    // builders
    Param* add_param(const std::string& key, std::vector<int64_t> shape, ParamKind kind, bool trainable);
    BN* add_bn(const std::string& prefix, int C, int bcast);
    void build_cba(Conv& L, const std::string& prefix, int nin, int nout_, int ks, int stride, int pad_h, int pad_w,
                   int dh, int dw, float slope);
    void build_basenet(BaseNetL& B, const std::string& prefix, int nin, int c, int nin_lstm, int nout_lstm_);
    void finalize_layout();

    // executor
    // `plain`: training only -- dense [N][C][Hv][Wv] copy of the values the conv sees (BatchNorm, activation,
    // dropout, upsample / broadcast applied), so that forward and weight gradient load it without arithmetic
    struct SrcSpec { Tensor t; bool up = false; int bcastH = 0; float* plain = nullptr; };
    // ---- training tape: forward order == topological order, backward walks it in reverse ----
    enum TapeKind { TK_CONV, TK_AVGPOOL, TK_SQUEEZE, TK_LSTM, TK_DENSE_ACT };
    struct TapeRec {
        TapeKind kind;
        Conv* L = nullptr;
        std::vector<SrcSpec> srcs;
        Tensor out;                  // raw output (+ g)
        int N = 0;
        bool batch_as_h = false;
        const float* bias = nullptr;
        Param* bias_param = nullptr;           // dense bias (gradient = channel sums of dz)
        LSTMMod* M = nullptr;                  // TK_LSTM / TK_SQUEEZE / TK_DENSE_ACT
        Tensor aux;                            // kind-specific second tensor
        float* save = nullptr;                 // LSTM gate/cell record
        float* buf0 = nullptr;                 // kind-specific buffers
        float* buf1 = nullptr;
        int chain = 0;                         // 1: high-band chain of stages 1-2 (independent of the low-band chain)
    };
    std::vector<TapeRec> tape;
    Arena gs;                                            // gradients of activations
    // First writer stores (round 4): the gradient buffer of a conv output is owned by that tensor alone -- every consumer's backward
    // addresses the whole tensor -- so the first backward writer STORES and the later ones accumulate: no zero fill, and the first
    // data-gradient epilogue writes instead of read-modify-writing zeros.  Buffers that are written through partial views (the
    // stage outputs aux1 / aux2: full tensor by stage 3, band halves by stage 2) or by kernels that only accumulate (pooled / LSTM
    // internals) stay zero-initialised: their byte ranges inside `gs` are recorded by the planning dry run (gs_zero).
    std::vector<std::pair<size_t, size_t>> gs_zero, gs_zero_plan;      // (offset, bytes); _plan = the dry run's list, what gets cleared
    std::map<const float*, bool> g_fresh;                // plain buffers of this forward: true until their first backward writer
    float* galloc(size_t n, bool plain);
    bool g_first(const float* g);                        // true exactly once per plain buffer: that writer must store, not accumulate
    void clear_gs_zero_ranges(hipStream_t st);
    float* g_arena = nullptr;                            // gradients of parameters (mirrors p_arena)
    float* m_arena = nullptr; float* v_arena = nullptr;  // Adam moments
    long long adam_step = 0;
    float* grad_of(const Param* p) { return p->grad_override ? p->grad_override : g_arena + (p->dev - p_arena); }
public:
    void debug_conv_bwd(const float* x, int N, int Cin, int H, int W, const float* w_oihw, int Cout, int KS, int stride,
                        int dh, int dw, int up, const float* aff, float slope, const float* dz, float* dx_out,
                        float* dw_out);
private:
    void ensure_train_state();
    void refresh_train_weights();
    template <class F> void plan_train_arenas(F&& dry_run, size_t extra_ws, bool clear_beside);
    void wait_gs_clear();                                // the main stream waits for a gs clear still running on lanes[0].main
    void backward();
    void bwd_conv(TapeRec& r);
    // which launches the data gradient of a conv record took (bwd_conv_dgrad's return value)
    enum DgradPath { DG_NONE = 0, DG_STRIDE1 = 1, DG_S2_FUSED = 2, DG_S2_CLASSES = 3, DG_S2_ZINS = 4 };
    int bwd_conv_dgrad(TapeRec& r, const ConvArgs& f);   // step 4 of bwd_conv; f = the record's forward launch (build_fwd_args)
    // The device forms of ONE layer's weights that its data gradient multiplies with, made from the K-major copy lc.P.dev
    // [Cin][KS*KS][CoutPad] of the local conv lc.L (dims set by the caller): flipped / transposed, their Winograd and plane forms in the
    // handle's mfma_mode, the four parity-class arrays of a stride-2 3x3.  Shared by debug_conv_bwd and the dgrad_launch hook of debug.hip.
    void debug_dgrad_weight_forms(LocalConv& lc);
    void bwd_bn_of(const Tensor& out, Conv& L);
    std::vector<float> dropout_host;                     // injected keep-masks [5][N][8*nout] or empty
    int dropout_mode = 1;                                // 0 off, 1 native RNG (default: nn.Dropout2d is active in train mode), 2 injected
    unsigned long long dropout_seed = 0x5DEECE66Dull;
    unsigned long long train_calls = 0;                  // counter of train-mode forwards: a fresh dropout draw for each (lib/layers.py:90)
    void prepare_dropout(int B);                         // fills dropout_dev for a train-mode forward of batch B
    float* dropout_buf = nullptr; size_t dropout_cap = 0;
public:
    // train.py:77-96: forward (train mode) + L1 loss + backward; gradients accumulate in the arena.
    void train_fwd_bwd_api(const float* X, const float* Y, bool on_dev, int B, int T, int accumulation_steps,
                           float* loss_out, float* mask_out, bool mask_on_dev);
    // the same step as two calls (autograd split): forward that keeps the graph, backward from dLoss/dmask
    void forward_train_api(const float* X, bool on_dev, int B, int T, float* mask_out, bool mask_on_dev);
    void backward_api(const float* dmask, bool on_dev);
    bool graph_valid = false; int graph_B = 0, graph_T = 0; Tensor graph_f3; float* graph_mask = nullptr;
    int64_t graph_gen = 0;                               // bumped by every vr_forward_train: the caller's backward names the graph it wants
    void param_arena(float** ptr, int64_t* numel) { *ptr = p_arena; *numel = (int64_t)p_floats; }
    void mark_params_dirty() { affine_dirty = true; }
    void adam_step_api(double lr, double b1, double b2, double eps, double grad_scale);
    void zero_grad_api();
    void adam_state(float* m_host, float* v_host, int64_t numel, int64_t* step, bool set);
    void get_grad(const std::string& key, float* host, int64_t cap_bytes);
    void set_dropout(int mode, unsigned long long seed, const float* masks, int B);
    void grad_arena(float** ptr, int64_t* numel);
    // ---- data-parallel exchange (comm.hip): RCCL on the handle's stream ----
    void comm_init(int rank, int world, const void* id128);
    void comm_destroy();
    void allreduce_grads(int wire_dtype);
    void broadcast_params(int root, bool with_optimizer);
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    void* wire_buf = nullptr;                            // bf16 copy of the gradient bucket (wire_dtype 1)
private:
    void build_fwd_args(Conv& L, const std::vector<SrcSpec>& srcs, int N, bool batch_as_h, ConvArgs& a);
    // A 1x1 stage that only reads what ONE conv stores, offered to that conv's run_conv: the stage tail behind a low-band dec1 (kind 1:
    // `L` into the view `out`; dec1's own output is then not written) or the LSTM squeeze behind dec2 (kind 2: `M` into out.p [N][H][W]).
    // run_conv takes it into the launch's epilogue (ConvArgs::tail) when option "fuse_tail" is on, in eval, mfma_mode 3, with no taps
    // recorded, and conv_x3h has the kernel for the launch's tiling (x3h_tail_ok); `done` says so, otherwise the caller launches it.
    struct FusedTail { int kind = 0; Conv* L = nullptr; LSTMMod* M = nullptr; Tensor out; bool done = false; };
    Tensor run_conv(Conv& L, const std::vector<SrcSpec>& srcs, int N, const Tensor* out_view, const float* bias,
                    bool batch_as_h, FusedTail* tail = nullptr);
    template <class F> void for_each_conv(F&& f);
    std::vector<Conv*> convs_;
    const std::vector<Conv*>& conv_layers();             // every conv in for_each_conv's order (train.hip)
    Tensor run_basenet(BaseNetL& B, const std::vector<SrcSpec>& in, int N, const Tensor* out_view, FusedTail* tail = nullptr);
    Tensor run_net_window(const Tensor& x, int w_lo, int w_hi);
    Tensor run_lstm(LSTMMod& M, const Tensor& h, float* z, bool squeezed);   // z: [N][h.H][h.W]; squeezed: dec2's launch has filled it
    SrcSpec upsampled(const Tensor& t);
    Tensor run_net(const Tensor& x);                     // -> stg3 dec1 output (raw + affine)
    // the network's input from X: an optional workspace copy (*copy: from where), a complex handle's pack, the strided tensor; dry: sizes only
    Tensor net_input(const float* X, const hipMemcpyKind* copy, int B, int T, const float** xd = nullptr);
    // the mask head of the handle's kind (sigmoid or complex) over the columns [w_lo, w_hi): to d.p / d.items, or dense to `out`
    void mask_head(const Tensor& f3, int w_lo, int w_hi, HeadDst d);
    void mask_head(const Tensor& f3, int w_lo, int w_hi, float* out);
    // ... of `cropsize`-wide crops: the columns [offset, cropsize - offset)
    void crop_mask_head(const Tensor& f3, int cropsize, HeadDst d);
    // `count` gathered crops, dense [count][nin][max_bin][cropsize] -> the network -> crop_mask_head
    void run_dense_crops(float* dense, int count, int cropsize, const HeadDst& d);
    struct StreamStepIO { const float* blk; long long blk_n, blk_pitch; float *y, *v; long long out_pitch, out_off; PcmIn pcm; };
    // One stream's share of a push call.  The caller fills S .. need (stream_check gives need); the rest is where stream_run stands.
    struct StreamPart {
        StreamState* S; const float* wave; long long n; bool flush; float *y, *v; long long capacity, need;
        long long at; bool flush_done; float *stage_in, *stage_y, *stage_v; StreamStepIO o;
        int channels, fmt;                                   // (PCM pushes) `wave` is bytes: frames of `channels` samples in format `fmt`
        std::vector<unsigned long long> st;                  // MEASURE, flush: the statistics rows on their way to S->coef
    };
    // The one executor of vr_stream_push (one part) and vr_stream_push_many: the steps of its parts in rounds, one set of launches per
    // round.  A step of one stream is stream_step_plan (takes the block in, asks stream_schedule what is ready, checks the rings and
    // fills the StreamSeg), its share of the round's launches, and stream_step_commit (flips the tail / carry buffers and moves the
    // stream's counters on).
    struct StreamStepPlan { StreamSeg seg; StreamSchedule p; int new_frames, segments, post_frames; bool emit, post_walk; };
    struct StreamCrop { int entry, pass; long long idx; };          // crop idx of a pass of the stream at table entry `entry`
    long long stream_check(const StreamState& S, const std::string& who, const float* wave, long long n, bool flush, const float* y,
                           const float* v, bool out_on_dev, long long capacity) const;     // -> samples per channel the call returns
    void stream_run(std::vector<StreamPart>& parts, int bs, bool on_dev, bool out_on_dev, bool pcm = false);
    StreamStepPlan stream_step_plan(StreamState& S, const StreamStepIO& io_, bool final);
    void stream_step_crops(const StreamState& S, const StreamStepPlan& sp, int entry, std::vector<StreamCrop>& list) const;
    void stream_step_commit(StreamState& S, StreamStepIO& io_, const StreamStepPlan& sp);
    void tap(const std::string& name, const Tensor& t);
    bool dry = false;
    const float* dropout_dev = nullptr;                  // [5][N][Cmax] keep-masks (training), or null
    void plan_and_reserve(int B, int T, size_t extra_bytes);
    void record_begin(int kind, double flops);
    void record_note(double bytes, const char* tag);
    double conv_alg_bytes(const Conv& L, const ConvArgs& a, int N, bool batch_as_h) const;
    void record_end();
};

}  // namespace vr
