// Host side of libvr_mi355.so: see model.h.  Topology follows lib/nets.py:8-141 and
// lib/layers.py:8-133 of the reference; parameter keys are the reference's state_dict keys.
#include "pcm.h"
#include "model.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace vr {

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// =====================================================================================================
// construction
// =====================================================================================================
Param* Model::add_param(const std::string& key, std::vector<int64_t> shape, ParamKind kind, bool trainable) {
    params.emplace_back();
    Param* p = &params.back();
    p->key = key;
    p->shape = std::move(shape);
    p->kind = kind;
    p->trainable = trainable;
    p->numel = 1;
    for (auto d : p->shape) p->numel *= (size_t)d;
    p->dev_numel = p->numel;
    if (kind == PK_CONV) {
        p->Cout = (int)p->shape[0];
        p->Cin = (int)p->shape[1];
        p->KK = p->shape.size() == 4 ? (int)(p->shape[2] * p->shape[3]) : 1;
        p->CoutPad = round_up(p->Cout, 32);
        p->dev_numel = (size_t)p->Cin * p->KK * p->CoutPad;
    }
    if (kind == PK_NBT) p->dev_numel = 0;
    by_key[key] = p;
    return p;
}

BN* Model::add_bn(const std::string& prefix, int C, int bcast) {
    bns.emplace_back();
    BN* b = &bns.back();
    b->C = C;
    b->bcast = bcast;
    b->w = add_param(prefix + ".weight", {C}, PK_PLAIN, true);
    b->b = add_param(prefix + ".bias", {C}, PK_PLAIN, true);
    b->rm = add_param(prefix + ".running_mean", {C}, PK_BUFFER, false);
    b->rv = add_param(prefix + ".running_var", {C}, PK_BUFFER, false);
    b->nbt = add_param(prefix + ".num_batches_tracked", {}, PK_NBT, false);
    bn_list.push_back(b);
    return b;
}

// layers.Conv2DBNActiv (lib/layers.py:8-26)
void Model::build_cba(Conv& L, const std::string& prefix, int nin, int nout_, int ks, int stride, int pad_h, int pad_w,
                      int dh, int dw, float slope) {
    L.name = prefix;
    L.Cin = nin; L.Cout = nout_; L.CoutPad = round_up(nout_, 32);
    L.KS = ks; L.stride = stride; L.pad_h = pad_h; L.pad_w = pad_w; L.dh = dh; L.dw = dw; L.slope = slope;
    L.w = add_param(prefix + ".conv.0.weight", {nout_, nin, ks, ks}, PK_CONV, true);
    L.bn = add_bn(prefix + ".conv.1", nout_, 0);
    L.cls = form_class(ks, stride, dh, dw, false);
}

// nets.BaseNet (lib/nets.py:10-24)
void Model::build_basenet(BaseNetL& B, const std::string& p, int nin, int c, int nin_lstm, int nout_lstm_) {
    B.prefix = p; B.c = c;
    const float RELU = 0.f, LEAKY = 0.01f;
    build_cba(B.enc1, p + ".enc1", nin, c, 3, 1, 1, 1, 1, 1, RELU);
    const int ch[5] = {c, 2 * c, 4 * c, 6 * c, 8 * c};
    for (int i = 0; i < 4; ++i) {
        const std::string e = p + ".enc" + std::to_string(i + 2);
        build_cba(B.enc_a[i], e + ".conv1", ch[i], ch[i + 1], 3, 2, 1, 1, 1, 1, LEAKY);
        build_cba(B.enc_b[i], e + ".conv2", ch[i + 1], ch[i + 1], 3, 1, 1, 1, 1, 1, LEAKY);
    }
    const int C8 = 8 * c;
    build_cba(B.aspp_pool, p + ".aspp.conv1.1", C8, C8, 1, 1, 0, 0, 1, 1, RELU);
    build_cba(B.aspp_c2, p + ".aspp.conv2", C8, C8, 1, 1, 0, 0, 1, 1, RELU);
    B.aspp_c2.cls = form_class(1, 1, 1, 1, true);                          // (runs beside the dilated branches in their launch)
    const int dil[3][2] = {{4, 2}, {8, 4}, {12, 6}};
    for (int i = 0; i < 3; ++i)
        build_cba(B.aspp_d[i], p + ".aspp.conv" + std::to_string(i + 3), C8, C8, 3, 1, dil[i][0], dil[i][1], dil[i][0],
                  dil[i][1], RELU);
    build_cba(B.aspp_bott, p + ".aspp.bottleneck", 5 * C8, C8, 1, 1, 0, 0, 1, 1, RELU);
    build_cba(B.dec[0], p + ".dec4.conv1", 14 * c, 6 * c, 3, 1, 1, 1, 1, 1, RELU);
    build_cba(B.dec[1], p + ".dec3.conv1", 10 * c, 4 * c, 3, 1, 1, 1, 1, 1, RELU);
    build_cba(B.dec[2], p + ".dec2.conv1", 6 * c, 2 * c, 3, 1, 1, 1, 1, 1, RELU);
    // layers.LSTMModule (lib/layers.py:110-122)
    LSTMMod& M = B.lstm;
    const std::string q = p + ".lstm_dec2";
    const int hid = nout_lstm_ / 2;
    M.nin = nin_lstm; M.hid = hid;
    M.squeeze.name = q + ".conv";
    M.squeeze.Cin = 2 * c; M.squeeze.Cout = 1; M.squeeze.KS = 1; M.squeeze.slope = RELU;
    M.squeeze.w = add_param(q + ".conv.conv.0.weight", {1, 2 * c, 1, 1}, PK_PLAIN, true);
    M.squeeze.bn = add_bn(q + ".conv.conv.1", 1, nin_lstm);
    M.proj.name = q + ".lstm";
    M.proj.Cin = nin_lstm; M.proj.Cout = 8 * hid; M.proj.CoutPad = round_up(8 * hid, 32);
    M.proj.KS = 1; M.proj.stride = 1; M.proj.pad_h = M.proj.pad_w = 0; M.proj.bn = nullptr; M.proj.slope = 1.f;
    Param* ihf = add_param(q + ".lstm.weight_ih_l0", {4 * hid, nin_lstm}, PK_LSTM_IH, true);
    M.whh_f = add_param(q + ".lstm.weight_hh_l0", {4 * hid, hid}, PK_PLAIN, true);
    M.b_ih_f = add_param(q + ".lstm.bias_ih_l0", {4 * hid}, PK_PLAIN, true);
    M.b_hh_f = add_param(q + ".lstm.bias_hh_l0", {4 * hid}, PK_PLAIN, true);
    Param* ihr = add_param(q + ".lstm.weight_ih_l0_reverse", {4 * hid, nin_lstm}, PK_LSTM_IH, true);
    M.whh_r = add_param(q + ".lstm.weight_hh_l0_reverse", {4 * hid, hid}, PK_PLAIN, true);
    M.b_ih_r = add_param(q + ".lstm.bias_ih_l0_reverse", {4 * hid}, PK_PLAIN, true);
    M.b_hh_r = add_param(q + ".lstm.bias_hh_l0_reverse", {4 * hid}, PK_PLAIN, true);
    ihf->Cout = 4 * hid; ihf->Cin = nin_lstm; ihf->KK = 1; ihf->CoutPad = M.proj.CoutPad; ihf->co_off = 0;
    ihf->dev_numel = (size_t)nin_lstm * M.proj.CoutPad;
    ihr->Cout = 4 * hid; ihr->Cin = nin_lstm; ihr->KK = 1; ihr->CoutPad = M.proj.CoutPad; ihr->co_off = 4 * hid;
    ihr->dev_numel = 0; ihr->alias_of = ihf;
    M.proj.w = ihf;
    M.dense.name = q + ".dense";
    M.dense.Cin = 2 * hid; M.dense.Cout = nin_lstm; M.dense.CoutPad = round_up(nin_lstm, 32);
    M.dense.KS = 1; M.dense.stride = 1; M.dense.pad_h = M.dense.pad_w = 0; M.dense.slope = 0.f;
    M.dense.w = add_param(q + ".dense.0.weight", {nin_lstm, 2 * hid}, PK_CONV, true);
    M.dense_b = add_param(q + ".dense.0.bias", {nin_lstm}, PK_PLAIN, true);
    M.dense.bn = add_bn(q + ".dense.1", nin_lstm, 0);
    build_cba(B.dec[3], p + ".dec1.conv1", 3 * c + 1, c, 3, 1, 1, 1, 1, 1, RELU);
}

Model::Model(int device_, int n_fft_, int hop_, int nout_, int nout_lstm_, bool is_complex_)
    : device(device_), n_fft(n_fft_), hop(hop_), nout(nout_), nout_lstm(nout_lstm_), is_complex(is_complex_), nin(is_complex_ ? 4 : 2) {
    VR_CHECK(n_fft >= 64 && (n_fft & (n_fft - 1)) == 0 && n_fft <= 8192, -2, "n_fft must be a power of two in [64, 8192]");
    VR_CHECK(hop > 0, -2, "hop_length must be positive");
    VR_CHECK(nout % 4 == 0 && nout >= 4 && nout_lstm % 4 == 0 && nout_lstm >= 4, -2, "nout / nout_lstm must be multiples of 4");
    max_bin = n_fft / 2;
    output_bin = n_fft / 2 + 1;
    VR_CHECK((max_bin / 2) % 16 == 0, -2, "n_fft/4 must be a multiple of 16 (four stride-2 encoders)");
    DeviceGuard dev_guard(device);
    if (const char* e = getenv("VR_MFMA_MODE")) { mfma_mode = atoi(e); VR_CHECK(mfma_mode >= 0 && mfma_mode <= 3, -2, "VR_MFMA_MODE: 0, 1, 2 or 3"); }
    default_mfma_mode = mfma_mode;
    VR_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (!getenv("VR_NO_SIDE_STREAM")) {
        VR_HIP(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
        VR_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        VR_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        if (!getenv("VR_NO_SPLIT_BATCH")) {
            int k = getenv("VR_LANES") ? atoi(getenv("VR_LANES")) : 2;
            k = k < 1 ? 1 : (k > 4 ? 4 : k);
            lanes.resize(k - 1);
            for (Lane& l : lanes) {
                VR_HIP(hipStreamCreateWithFlags(&l.main, hipStreamNonBlocking));
                VR_HIP(hipStreamCreateWithFlags(&l.side, hipStreamNonBlocking));
                VR_HIP(hipEventCreateWithFlags(&l.fork, hipEventDisableTiming));
                VR_HIP(hipEventCreateWithFlags(&l.join, hipEventDisableTiming));
                VR_HIP(hipEventCreateWithFlags(&l.start, hipEventDisableTiming));
                VR_HIP(hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
            }
        }
    }
    const int nin_lstm = max_bin / 2;
    // lib/nets.py:59-80
    build_basenet(nets_[0], "stg1_low_band_net.0", nin, nout / 2, nin_lstm / 2, nout_lstm);
    build_cba(tail1, "stg1_low_band_net.1", nout / 2, nout / 4, 1, 1, 0, 0, 1, 1, 0.f);
    build_basenet(nets_[1], "stg1_high_band_net", nin, nout / 4, nin_lstm / 2, nout_lstm / 2);
    build_basenet(nets_[2], "stg2_low_band_net.0", nout / 4 + nin, nout, nin_lstm / 2, nout_lstm);
    build_cba(tail2, "stg2_low_band_net.1", nout, nout / 2, 1, 1, 0, 0, 1, 1, 0.f);
    build_basenet(nets_[3], "stg2_high_band_net", nout / 4 + nin, nout / 2, nin_lstm / 2, nout_lstm / 2);
    build_basenet(nets_[4], "stg3_full_band_net", 3 * nout / 4 + nin, nout, nin_lstm, nout_lstm);
    out_w = add_param("out.weight", {nin, nout, 1, 1}, PK_PLAIN, true);
    aux_out_w = add_param("aux_out.weight", {nin, 3 * nout / 4, 1, 1}, PK_PLAIN, true);   // never used (nets.py:80)
    finalize_layout();

    fft_plan_create(plan, n_fft);
}

// FFT plan: twiddles and periodic Hann window computed in double on the host
void fft_plan_create(FFTPlan& plan, int n_fft) {
    FFTPlan p{};
    p.n_fft = n_fft;
    while ((1 << p.log2n) < n_fft) ++p.log2n;
    std::vector<float2> tw(n_fft / 2);
    std::vector<float> win(n_fft);
    const double PI = 3.14159265358979323846;
    for (int k = 0; k < n_fft / 2; ++k) {
        const double a = -2.0 * PI * k / n_fft;
        tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int i = 0; i < n_fft; ++i) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * i / n_fft));
    try {
        VR_HIP(hipMalloc(&p.twiddle, tw.size() * sizeof(float2)));
        VR_HIP(hipMalloc(&p.window, win.size() * sizeof(float)));
        VR_HIP(hipMemcpy(p.twiddle, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        VR_HIP(hipMemcpy(p.window, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
    } catch (...) {                                      // `plan` is left as it was: never an n_fft without its tables
        hipFree(p.twiddle); hipFree(p.window);
        throw;
    }
    plan = p;
}

void Model::finalize_layout() {
    size_t poff = 0, boff = 0;
    auto bump = [](size_t& o, size_t n) { size_t a = (o + 63) & ~size_t(63); o = a + n; return a; };
    for (auto& p : params) {
        if (p.kind == PK_NBT || p.alias_of) continue;
        if (p.trainable) p.off = bump(poff, p.dev_numel);
        else p.off = bump(boff, p.dev_numel);
    }
    // BatchNorm affine tables + saved batch statistics live in the buffer arena
    std::vector<size_t> aff_off(bn_list.size()), sm_off(bn_list.size()), si_off(bn_list.size());
    for (size_t i = 0; i < bn_list.size(); ++i) {
        BN* b = bn_list[i];
        const int rows = b->bcast ? b->bcast : b->C;
        aff_off[i] = bump(boff, (size_t)rows * 2);
        sm_off[i] = bump(boff, (size_t)b->C);
        si_off[i] = bump(boff, (size_t)b->C);
    }
    size_t aspp_off[5];
    for (int i = 0; i < 5; ++i) aspp_off[i] = bump(boff, (size_t)4 * 8 * nets_[i].c * 2);
    p_floats = poff + 64; b_floats = boff + 64;
    VR_HIP(hipMalloc(&p_arena, p_floats * sizeof(float)));
    VR_HIP(hipMalloc(&b_arena, b_floats * sizeof(float)));
    VR_HIP(hipMemset(p_arena, 0, p_floats * sizeof(float)));
    VR_HIP(hipMemset(b_arena, 0, b_floats * sizeof(float)));
    for (auto& p : params) {
        if (p.kind == PK_NBT || p.alias_of) continue;
        p.dev = (p.trainable ? p_arena : b_arena) + p.off;
    }
    for (auto& p : params)
        if (p.alias_of) p.dev = p.alias_of->dev;
    for (size_t i = 0; i < bn_list.size(); ++i) {
        bn_list[i]->affine = b_arena + aff_off[i];
        bn_list[i]->save_mean = b_arena + sm_off[i];
        bn_list[i]->save_invstd = b_arena + si_off[i];
    }
    for (int i = 0; i < 5; ++i) {
        BaseNetL& B = nets_[i];
        B.aspp_aff = b_arena + aspp_off[i];
        const size_t blk = (size_t)8 * B.c * 2;
        B.aspp_c2.bn->affine = B.aspp_aff;
        for (int j = 0; j < 3; ++j) B.aspp_d[j].bn->affine = B.aspp_aff + (j + 1) * blk;
    }
    // default BatchNorm state = torch's fresh module: weight 1, running_var 1
    for (BN* b : bn_list) {
        std::vector<float> ones(b->C, 1.f);
        VR_HIP(hipMemcpy(b->w->dev, ones.data(), b->C * sizeof(float), hipMemcpyHostToDevice));
        VR_HIP(hipMemcpy(b->rv->dev, ones.data(), b->C * sizeof(float), hipMemcpyHostToDevice));
    }
    std::vector<BNFoldDesc> descs;
    for (BN* b : bn_list) descs.push_back(BNFoldDesc{b->w->dev, b->b->dev, b->rm->dev, b->rv->dev, b->affine, b->C, b->bcast});
    VR_HIP(hipMalloc(&d_fold, descs.size() * sizeof(BNFoldDesc)));
    VR_HIP(hipMemcpy(d_fold, descs.data(), descs.size() * sizeof(BNFoldDesc), hipMemcpyHostToDevice));
    affine_dirty = true;
}

Model::~Model() {
    if (launch_prof && !prof_owned_by_this_thread(launch_prof)) prof_abandon(launch_prof);   // the opening thread still holds the pointer
    else { if (g_launch_prof == launch_prof) g_launch_prof = nullptr; prof_destroy(launch_prof); }
    int prev_dev = -1;
    if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
    hipSetDevice(device);
    struct Back { int d; ~Back() { if (d >= 0) hipSetDevice(d); } } back{prev_dev};
    try { comm_destroy(); } catch (...) {}
    hipFree(wire_buf);
    if (stream) hipStreamSynchronize(stream);
    hipFree(p_arena); hipFree(b_arena); hipFree(d_fold);
    hipFree(ws.base); hipFree(io.base); hipFree(gs.base); form_store.release(); hipFree(aug_buf); hipFree(wred_dev);
    for (BaseNetL& B : nets_) hipFree(B.lstm.bias_sum);
    hipFree(g_arena); hipFree(m_arena); hipFree(v_arena); hipFree(dropout_buf);
    hipFree(plan.twiddle); hipFree(plan.window);
    hipFree(shift_plan.twiddle); hipFree(shift_plan.window);
    for (Lane& l : lanes) {
        hipStreamSynchronize(l.main); hipStreamSynchronize(l.side);
        hipStreamDestroy(l.main); hipStreamDestroy(l.side);
        hipEventDestroy(l.fork); hipEventDestroy(l.join); hipEventDestroy(l.start); hipEventDestroy(l.done);
        hipFree(l.ws.base);
    }
    if (side_stream) { hipStreamSynchronize(side_stream); hipStreamDestroy(side_stream); hipEventDestroy(ev_fork); hipEventDestroy(ev_join); }
    if (stream) hipStreamDestroy(stream);
}

// =====================================================================================================
// parameters
// =====================================================================================================
void Model::set_param(const std::string& key, const void* host, const int64_t* shape, int ndim) {
    auto it = by_key.find(key);
    VR_CHECK(it != by_key.end(), -2, "unknown parameter key: " + key);
    Param& p = *it->second;
    VR_CHECK((size_t)ndim == p.shape.size(), -2, "shape rank mismatch for " + key);
    for (int i = 0; i < ndim; ++i) VR_CHECK(shape[i] == p.shape[i], -2, "shape mismatch for " + key);
    DeviceGuard dev_guard(device);
    VR_HIP(hipStreamSynchronize(stream));
    if (p.kind == PK_NBT) { p.nbt = *static_cast<const int64_t*>(host); return; }
    const float* src = static_cast<const float*>(host);
    if (p.kind == PK_CONV) {
        std::vector<float> tmp((size_t)p.Cin * p.KK * p.CoutPad, 0.f);
        for (int co = 0; co < p.Cout; ++co)
            for (int ci = 0; ci < p.Cin; ++ci)
                for (int k = 0; k < p.KK; ++k)
                    tmp[((size_t)ci * p.KK + k) * p.CoutPad + co] = src[((size_t)co * p.Cin + ci) * p.KK + k];
        VR_HIP(hipMemcpy(p.dev, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice));
    } else if (p.kind == PK_LSTM_IH) {
        std::vector<float> tmp((size_t)p.Cin * p.Cout);
        for (int co = 0; co < p.Cout; ++co)
            for (int ci = 0; ci < p.Cin; ++ci) tmp[(size_t)ci * p.Cout + co] = src[(size_t)co * p.Cin + ci];
        VR_HIP(hipMemcpy2D(p.dev + p.co_off, (size_t)p.CoutPad * sizeof(float), tmp.data(), (size_t)p.Cout * sizeof(float),
                           (size_t)p.Cout * sizeof(float), (size_t)p.Cin, hipMemcpyHostToDevice));
    } else {
        VR_HIP(hipMemcpy(p.dev, src, p.numel * sizeof(float), hipMemcpyHostToDevice));
    }
    affine_dirty = true;
}

void Model::get_param(const std::string& key, void* host, int64_t cap_bytes) {
    auto it = by_key.find(key);
    VR_CHECK(it != by_key.end(), -2, "unknown parameter key: " + key);
    Param& p = *it->second;
    DeviceGuard dev_guard(device);
    VR_HIP(hipStreamSynchronize(stream));
    if (p.kind == PK_NBT) {
        VR_CHECK(cap_bytes >= 8, -2, "buffer too small");
        *static_cast<int64_t*>(host) = p.nbt;
        return;
    }
    VR_CHECK((size_t)cap_bytes >= p.numel * sizeof(float), -2, "buffer too small for " + key);
    float* dst = static_cast<float*>(host);
    if (p.kind == PK_CONV) {
        std::vector<float> tmp((size_t)p.Cin * p.KK * p.CoutPad);
        VR_HIP(hipMemcpy(tmp.data(), p.dev, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int co = 0; co < p.Cout; ++co)
            for (int ci = 0; ci < p.Cin; ++ci)
                for (int k = 0; k < p.KK; ++k)
                    dst[((size_t)co * p.Cin + ci) * p.KK + k] = tmp[((size_t)ci * p.KK + k) * p.CoutPad + co];
    } else if (p.kind == PK_LSTM_IH) {
        std::vector<float> tmp((size_t)p.Cin * p.Cout);
        VR_HIP(hipMemcpy2D(tmp.data(), (size_t)p.Cout * sizeof(float), p.dev + p.co_off, (size_t)p.CoutPad * sizeof(float),
                           (size_t)p.Cout * sizeof(float), (size_t)p.Cin, hipMemcpyDeviceToHost));
        for (int co = 0; co < p.Cout; ++co)
            for (int ci = 0; ci < p.Cin; ++ci) dst[(size_t)co * p.Cin + ci] = tmp[(size_t)ci * p.Cout + co];
    } else {
        VR_HIP(hipMemcpy(dst, p.dev, p.numel * sizeof(float), hipMemcpyDeviceToHost));
    }
}

void Model::need_real_mask(const char* what) const {
    VR_CHECK(!is_complex || complex_train, -2, std::string(what) + ": this handle predicts a complex mask (is_complex=True); only eval-mode inference "
                              "is supported for it, training is not");
}

void Model::need_real_mask_train(const char* what) const {
    VR_CHECK(!(is_complex && training) || complex_train, -2, std::string(what) + " in training mode: this handle predicts a complex mask "
                                            "(is_complex=True); only eval-mode inference is supported for it, training is not");
}

void Model::set_training(bool t) {
    if (training && !t) affine_dirty = true;     // batch-stat affines must be replaced by running-stat ones
    training = t;
}

void Model::fold_eval_affines() {
    if (!affine_dirty) return;
    int maxC = 1;
    for (BN* b : bn_list) maxC = std::max(maxC, std::max(b->C, b->bcast));
    launch_bn_fold_eval(d_fold, (int)bn_list.size(), maxC, 1e-5f, stream);
    refresh_forms(false);       // the weights may have changed too (set_param / Adam)
    for (BaseNetL& B : nets_) {  // LSTM gate biases b_ih + b_hh, once per parameter change instead of two launches per LSTM and forward
        LSTMMod& M = B.lstm;
        const int G = 4 * M.hid;
        if (!M.bias_sum) VR_HIP(hipMalloc(reinterpret_cast<void**>(&M.bias_sum), (size_t)2 * G * sizeof(float)));
        launch_add(M.b_ih_f->dev, M.b_hh_f->dev, M.bias_sum, G, stream);
        launch_add(M.b_ih_r->dev, M.b_hh_r->dev, M.bias_sum + G, G, stream);
    }
    affine_dirty = false;
}

void Model::set_option(const std::string& name, int value) {
    plan_peak = 0;                                           // kernel choice and scratch layout depend on the options: re-plan the next forward
    if (name == "train_winograd") train_wino = value != 0;
    else if (name == "serial_exec") serial = value != 0;     // every kernel on the handle's one stream (race detector of the tests)
    else if (name == "params_dirty") affine_dirty = true;    // the parameter arena was written from outside (vr_param_arena)
    else if (name == "mfma_bf16") { mfma_mode = value != 0 ? 1 : default_mfma_mode; affine_dirty = true; }   // bf16 operands on the matrix pipe (0: back to the handle's default mode)
    else if (name == "mfma_mode") {                          // 0 fp32 MFMA, 1 bf16 operands, 2 fp32 via 6 bf16 products, 3 via 3 fp16 products (model.h); -1 = the default
        if (value < -1 || value > 3) throw Error(-2, "mfma_mode: 0, 1, 2, 3 or -1 (default)");
        mfma_mode = value < 0 ? default_mfma_mode : value; affine_dirty = true;   // (the next eval forward refreshes the derived weight copies)
    }
    else if (name == "conv_x3d") {                           // the 16-column layers on the fp16 pipe (conv_x3d.hip, mfma_mode 3): 0 off (conv_dma.hip as in round 5),
        if (value < -1 || value > 2) throw Error(-2, "conv_x3d: 0, 1, 2 or -1 (default)");     // 1 one launch per conv, 2 (default) + the four ASPP branches in one launch
        x3d_mode = value < 0 ? 2 : value;
    }
    else if (name == "conv_x3s") {                           // the 3x3 stride-2 layers on the fp16 pipe in eval (conv_x3s.hip, mfma_mode 3): 0 off (conv_dma.hip)
        if (value < -1 || value > 1) throw Error(-2, "conv_x3s: 0, 1 or -1 (default)");
        x3s_mode = value < 0 ? x3s_default() : value;
    }
    else if (name == "crop_window") crop_window = value != 0;
    else if (name == "fuse_tail") fuse_tail = value != 0;
    else if (name == "lstm_gemm") lstm_gemm = value != 0;
    else if (name == "aspp_pool_fused") aspp_pool_fused = value != 0;
    else if (name == "complex_train") {                      // a complex handle under the training entry points (off by default: they refuse it)
        if (!is_complex) throw Error(-2, "complex_train: this handle predicts a magnitude mask; the option belongs to complex-mask handles (VR_CREATE_COMPLEX)");
        complex_train = value != 0;
        if (!complex_train && loss_kind != 0) set_loss(0, 0.01);          // VR_LOSS_MAG_L1_WAVE_SDR lives on complex training only
        graph_valid = false;
    }
    else if (name == "adam_reset") reset_adam_state();      // a freshly constructed torch.optim.Adam has no moments
    else if (name == "hip_graph" || name == "conv_x3p" || name == "wgrad_x3h" || name == "conv_x3b") {
        // options of round 4 whose kernels moved to tools/experiments in round 5: accepted and ignored, so that an older caller keeps
        // working; said once per option name
        static std::string told;
        if (told.find("|" + name + "|") == std::string::npos) {
            told += "|" + name + "|";
            fprintf(stderr, "libvr_mi355: option '%s' was retired with its kernel (tools/experiments/README.md); ignored\n", name.c_str());
        }
    }
    else throw Error(-2, "unknown option: " + name);
}

// One allocation for form `f` of `convs`: total -> hipMalloc -> offsets into the layers' records.  Once per store and form; wt is zero
// filled here and never again (the flip kernel does not write its ci >= Cin padding).
void Model::hold_form(FormId f, const std::vector<Conv*>& convs, Wino6Want w6, FormStore& s) {
    if (s.arena[f]) return;
    auto room = [&](const Conv* L) {
        const FormSpec sp = form_spec(f, *L, mfma_mode, w6);
        return sp.held ? (sp.bytes + 255) & ~size_t(255) : size_t(0);
    };
    size_t total = 0;
    for (const Conv* L : convs) total += room(L);
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&s.arena[f]), total ? total : 16));
    if (f == F_WT) {
        VR_HIP(hipMemset(s.arena[f], 0, total));
        VR_HIP(hipStreamSynchronize(nullptr));                // (the fill runs on the NULL stream, the transforms on the handle's)
    }
    size_t off = 0;
    for (Conv* L : convs)
        if (room(L)) { L->forms.p[f] = s.arena[f] + off; off += room(L); }
}

// Form `f` of every conv that holds it and whose image mfma_mode reads: one batched launch from the form's descriptor table, or
// (`single`, the hooks) one single-layer launch per conv where such a launcher exists.  The table is made when the mode changes: the
// pointers and dims of a held form never do.
void Model::fill_form(FormId f, const std::vector<Conv*>& convs, Wino6Want w6, FormStore& s, bool single) {
    FormStore::Tables& t = s.tbl[f];
    const bool split6 = f == F_WINO6 || f == F_WINOT6, planes = f == F_X3W || f == F_X3T;
    if (t.mode != mfma_mode) {
        std::vector<WinoWDesc> wd;
        std::vector<X3WDesc> xd;
        std::vector<FlipDesc> fd;
        std::vector<S2WDesc> sd;
        for (Conv* L : convs) {
            const FormSpec sp = form_spec(f, *L, mfma_mode, w6);
            if (!sp.held || !sp.live) continue;
            const float* src = sp.from_wt ? L->forms.f32(F_WT) : L->w->dev;
            void* dst = L->forms.p[f];
            if (f == F_WT) fd.push_back(FlipDesc{src, static_cast<float*>(dst), L->Cin, L->Cout, sp.KK, sp.pad, L->CoutPad});
            else if (f == F_S2W) sd.push_back(S2WDesc{src, static_cast<float*>(dst), L->Cin, L->Cout, L->CoutPad, sp.pad});
            else if (!single) { if (planes) xd.push_back(X3WDesc{src, dst, sp.rows, sp.KK, sp.pad}); else wd.push_back(WinoWDesc{src, dst, sp.rows, sp.pad}); }
            else if (planes && mfma_mode == 3) launch_x3h_weights(src, dst, sp.rows, sp.KK, sp.pad, stream);
            else if (planes) launch_x3_weights(src, dst, sp.rows, sp.KK, sp.pad, stream);
            else if (split6) launch_wino_weights6(src, dst, sp.rows, sp.pad, stream);
            else launch_wino_weights(src, static_cast<float*>(dst), sp.rows, sp.pad, stream);
        }
        t.n = (int)(fd.size() + sd.size() + wd.size() + xd.size());
        if (!fd.empty()) t.flip.upload(fd, stream);
        if (!sd.empty()) { t.s2.upload(sd, stream); t.max_elems = s2w_batch_max_elems(sd); }
        if (!wd.empty()) { t.wino.upload(wd, stream); t.max_elems = wino_batch_max_elems(wd, split6); }
        if (!xd.empty()) { t.x3.upload(xd, stream); t.max_elems = x3_batch_max_elems(xd); t.max_cout_pad = x3_batch_max_cout_pad(xd); }
        t.mode = mfma_mode;
    }
    if (!t.n) return;
    if (f == F_WT) launch_flip_transpose(t.flip.dev, t.n, stream);
    else if (f == F_S2W) launch_s2_class_weights(t.s2.dev, t.n, t.max_elems, stream);
    else if (!planes) launch_wino_weights_batched(t.wino.dev, t.n, t.max_elems, split6, stream);
    else if (mfma_mode == 3) launch_x3h_weights_batched(t.x3.dev, t.n, t.max_elems, t.max_cout_pad, stream);
    else launch_x3_weights_batched(t.x3.dev, t.n, t.max_elems, stream);
}

// The handle's refresh: the forward forms of the current mfma_mode; with_dgrad (once per train step): first wt and the parity classes,
// then the forms made from wt.  A form is allocated when a refresh first fills it.
void Model::refresh_forms(bool with_dgrad) {
    static const bool x3_on = !(getenv("VR_CONV_X3") && atoi(getenv("VR_CONV_X3")) == 0);
    // split-bf16 (mode 2) / split-fp16 (mode 3) planes of the direct weights; VR_CONV_X3=0 in mode 2: bf16 planes of U instead, for the
    // launches that can take the split kernel -- the 64-cout Winograd variant only (conv_wino.hip)
    const bool x3 = x3_mode() && x3_on, six = mfma_mode == 2 && !x3_on;
    bool fill[F_COUNT] = {};
    fill[F_WINO] = true; fill[F_WINO6] = six; fill[F_X3W] = x3;
    fill[F_WT] = fill[F_S2W] = fill[F_WINOT] = with_dgrad; fill[F_WINOT6] = with_dgrad && six; fill[F_X3T] = with_dgrad && x3;
    for (FormId f : {F_WT, F_S2W, F_WINO, F_WINO6, F_X3W, F_WINOT, F_WINOT6, F_X3T}) {
        if (!fill[f]) continue;
        hold_form(f, conv_layers(), W6_PAD64, form_store);
        fill_form(f, conv_layers(), W6_PAD64, form_store, false);
    }
}

long long Model::x3_batch_max_elems(const std::vector<X3WDesc>& descs) {
    long long m = 0;
    for (const X3WDesc& e : descs) m = std::max(m, (long long)((e.Cin + 7) / 8 * 8) * e.KK * e.CoutPad);
    return m;
}
int Model::x3_batch_max_cout_pad(const std::vector<X3WDesc>& descs) {
    int mc = 0;
    for (const X3WDesc& e : descs) mc = std::max(mc, e.CoutPad);
    return mc;
}
long long Model::wino_batch_max_elems(const std::vector<WinoWDesc>& descs, bool split6) {
    long long m = 0;
    for (const WinoWDesc& e : descs) {
        const long long cin = split6 ? (e.Cin + 7) / 8 * 8 : e.Cin;
        m = std::max(m, cin * e.CoutPad);
    }
    return m;
}
long long Model::s2w_batch_max_elems(const std::vector<S2WDesc>& descs) {
    long long m = 0;
    for (const S2WDesc& e : descs) m = std::max(m, (long long)4 * e.Cout * 9 * e.CinPad);
    return m;
}

// =====================================================================================================
// workspace
// =====================================================================================================
void Model::ensure_ws(size_t bytes) {
    if (bytes <= ws.cap) return;
    VR_HIP(hipStreamSynchronize(stream));
    if (ws.base) VR_HIP(hipFree(ws.base));
    ws.base = nullptr; ws.cap = 0;
    const size_t want = bytes + (bytes >> 4) + (1 << 20);
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&ws.base), want));
    ws.cap = want;
}

// Exchange lane A (stream, side_stream, ws) with lane B: run_net() and the launch helpers only know the
// member names, so the second half-batch is enqueued by swapping, running, swapping back.
void Model::swap_lane(int i) {
    Lane& l = lanes[i];
    std::swap(stream, l.main);
    std::swap(side_stream, l.side);
    std::swap(ev_fork, l.fork);
    std::swap(ev_join, l.join);
    std::swap(ws, l.ws);
}

void Model::ensure_io(size_t bytes) {
    if (bytes <= io.cap) return;
    VR_HIP(hipStreamSynchronize(stream));
    if (io.base) VR_HIP(hipFree(io.base));
    io.base = nullptr; io.cap = 0;
    const size_t want = bytes + (bytes >> 4) + (1 << 20);
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&io.base), want));
    io.cap = want;
}

// Algorithmic HBM bytes of one convolution launch -- forward, data gradient or weight gradient alike: the (virtual) input-sized
// tensor, the output-sized tensor and the weights, each crossing HBM once.
double Model::conv_alg_bytes(const Conv& L, const ConvArgs& a, int N, bool batch_as_h) const {
    return 4.0 * ((double)a.N * L.Cin * a.Hin * a.Win + (double)N * L.Cout * (batch_as_h ? 1 : a.Hout) * a.Wout +
                  (double)L.Cin * L.KS * L.KS * L.Cout);
}

// The executor's note for the next launch: a convolution's algorithmic FLOPs (bytes / tag follow through record_note).
void Model::record_begin(int kind, double flops) {
    if (!profiling || dry) return;
    (void)kind;
    prof_note(flops, 0.0, true, "conv");
}
void Model::record_note(double bytes, const char* tag) {
    if (!profiling || dry || !g_launch_prof) return;
    prof_note_update(bytes, tag);
}
void Model::record_end() {
    if (!profiling || dry) return;
    prof_note_clear();                                   // (a dispatcher that launched nothing leaves no stale note)
}

void Model::profile_begin() {
    VR_CHECK(!launch_prof || prof_owned_by_this_thread(launch_prof), -3, "vr_profile_begin: a profile opened by another thread is still open");
    prof_destroy(launch_prof);
    launch_prof = prof_create();
    g_launch_prof = launch_prof;
    profiling = true;
}

void Model::profile_end(double* conv_ms, double* conv_flops, double* conv_bytes, int* launches) {
    DeviceGuard dev_guard(device);
    VR_CHECK(!launch_prof || prof_owned_by_this_thread(launch_prof), -3, "vr_profile_end must be called from the thread that called vr_profile_begin");
    VR_HIP(hipDeviceSynchronize());                      // every stream the profiled step used
    g_launch_prof = nullptr;
    profiling = false;
    static const bool dump = getenv("VR_PROFILE_DUMP") != nullptr;           // per-launch table on stderr
    if (launch_prof) prof_collect(launch_prof, conv_ms, conv_flops, conv_bytes, launches, &profile_report, dump);
    prof_destroy(launch_prof);
    launch_prof = nullptr;
}

float* Model::galloc(size_t n, bool plain) {
    const size_t off = (gs.off + 255) & ~size_t(255);            // (Arena::alloc's own rounding)
    float* p = gs.allocf(n);
    if (!plain) gs_zero.push_back({off, n * sizeof(float)});
    else if (!dry) g_fresh[p] = true;
    return p;
}

bool Model::g_first(const float* g) {
    auto it = g_fresh.find(g);
    if (it == g_fresh.end() || !it->second) return false;
    it->second = false;
    return true;
}

// zero the buffers of `gs` that need it (ranges recorded by the planning dry run; adjacent ones merged)
void Model::clear_gs_zero_ranges(hipStream_t st) {
    // VR_GS_POISON=1 (debug): every byte of the arena is first set to 0xFF (a NaN pattern), so a backward writer that ACCUMULATES into a
    // buffer nobody stored to first (first-writer-stores keys g_fresh by the exact base pointer: an offset or partial view would get
    // g_first() == false) turns its tensor into NaNs instead of silently adding to last step's values -- the train-parity tests run
    // once under it (tests/test_gpu_train.py)
    static const bool poison = [] { const char* e = getenv("VR_GS_POISON"); return e && atoi(e) != 0; }();
    if (poison && gs.base && gs.cap) VR_HIP(hipMemsetAsync(gs.base, 0xFF, gs.cap, st));
    size_t i = 0;
    while (i < gs_zero_plan.size()) {
        size_t b = gs_zero_plan[i].first, e = b + gs_zero_plan[i].second;
        size_t j = i + 1;
        while (j < gs_zero_plan.size() && gs_zero_plan[j].first <= ((e + 255) & ~size_t(255))) {
            e = std::max(e, gs_zero_plan[j].first + gs_zero_plan[j].second);
            ++j;
        }
        prof_memset_async(gs.base + b, 0, e - b, st);
        i = j;
    }
}

void Model::tap(const std::string& name, const Tensor& t) {
    if (record_taps && !dry) taps[name] = t;
}

int64_t Model::get_tap(const std::string& name, float* host, int64_t cap_floats, int64_t* shape4) {
    DeviceGuard dev_guard(device);
    auto it = taps.find(name);
    VR_CHECK(it != taps.end(), -2, "no such tap: " + name);
    const Tensor& t = it->second;
    const int64_t n = (int64_t)t.N * t.C * t.H * t.W;
    if (shape4) { shape4[0] = t.N; shape4[1] = t.C; shape4[2] = t.H; shape4[3] = t.W; }
    if (!host) return n;
    VR_CHECK(cap_floats >= n, -2, "tap buffer too small");
    float* tmp = nullptr;
    VR_HIP(hipMalloc(&tmp, n * sizeof(float)));
    launch_materialize(t, tmp, stream);
    VR_HIP(hipStreamSynchronize(stream));
    VR_HIP(hipMemcpy(host, tmp, n * sizeof(float), hipMemcpyDeviceToHost));
    VR_HIP(hipFree(tmp));
    return n;
}

// =====================================================================================================
// executor
// =====================================================================================================
ConvSrc make_src(const Tensor& t, bool up, int bcastH) {
    ConvSrc s{};
    s.p = t.p; s.aff0 = t.aff0; s.aff1 = t.aff1 ? t.aff1 : t.aff0;
    s.sN = t.sN; s.sC = t.sC; s.sH = t.sH;
    s.C = t.C; s.H = t.H; s.W = t.W;
    s.hsplit = t.hsplit; s.slope = t.slope; s.up = up ? 1 : 0; s.post = t.post; s.zins = 0;
    s.rh = (t.H > 0) ? (float)(t.H - 1) / (float)(2 * t.H - 1) : 0.f;
    s.rw = (t.W > 0) ? (float)(t.W - 1) / (float)(2 * t.W - 1) : 0.f;
    if (bcastH) { s.sH = 0; s.H = bcastH; }
    return s;
}

// Forward launch description of a conv layer (shared by the forward pass and the weight gradient).
void Model::build_fwd_args(Conv& L, const std::vector<SrcSpec>& srcs, int N, bool batch_as_h, ConvArgs& a) {
    VR_CHECK(!srcs.empty() && srcs.size() <= 3, -2, "conv " + L.name + ": 1..3 sources");
    a = ConvArgs{};
    a.nsrc = (int)srcs.size();
    int Hin = -1, Win = -1, ctot = 0;
    for (int i = 0; i < a.nsrc; ++i) {
        const SrcSpec& sp = srcs[i];
        a.src[i] = make_src(sp.t, sp.up, sp.bcastH);
        const int vh = sp.up ? 2 * sp.t.H : (sp.bcastH ? sp.bcastH : sp.t.H);
        const int vw = sp.up ? 2 * sp.t.W : sp.t.W;
        if (sp.plain) {                       // materialised view of the same values
            ConvSrc& c = a.src[i];
            c = ConvSrc{};
            c.p = sp.plain; c.C = sp.t.C; c.H = vh; c.W = vw;
            c.sH = vw; c.sC = (long long)vh * vw; c.sN = c.sC * sp.t.C;
            c.hsplit = 1 << 30; c.slope = 1.f;
        }
        if (Hin < 0) { Hin = vh; Win = vw; }
        // spec_utils.crop_center (lib/spec_utils.py:8-23) is the identity for every valid shape;
        // anything else is the reference's ValueError.
        VR_CHECK(vh == Hin && vw == Win, -5, "h1_shape[3] must be greater than h2_shape[3] (decoder skip/upsample size mismatch in " + L.name + ")");
        ctot += sp.t.C;
    }
    VR_CHECK(ctot == L.Cin, -2, "conv " + L.name + ": channel count mismatch");
    {   // the loader keeps ONE interpolation table per workgroup: upsampled sources must share geometry
        const ConvSrc* u = nullptr;
        for (int i = 0; i < a.nsrc; ++i) {
            if (!a.src[i].up) continue;
            if (u) VR_CHECK(u->H == a.src[i].H && u->W == a.src[i].W && u->sH == a.src[i].sH, -2,
                            "conv " + L.name + ": upsampled sources must share H, W and row stride");
            u = &a.src[i];
        }
    }
    a.c1 = a.nsrc >= 2 ? srcs[0].t.C : L.Cin;
    a.c2 = a.nsrc >= 3 ? srcs[0].t.C + srcs[1].t.C : L.Cin;
    a.Cin = L.Cin;
    a.w = L.w->dev;
    a.Cout = L.Cout; a.CoutPad = L.CoutPad;
    a.d1 = a.d2 = 1 << 30;
    int Nk = N;
    if (batch_as_h) {
        VR_CHECK(L.KS == 1 && Hin == 1, -2, "batch-as-rows view needs a 1x1 conv on H=1 input");
        for (int i = 0; i < a.nsrc; ++i) {
            VR_CHECK(!a.src[i].post && !a.src[i].up, -2, "batch-as-rows: unsupported source flags");
            a.src[i].sH = a.src[i].sN; a.src[i].sN = 0; a.src[i].H = N;
        }
        Hin = N; Nk = 1;
    }
    a.N = Nk; a.Hin = Hin; a.Win = Win;
    a.Hout = (Hin + 2 * L.pad_h - L.dh * (L.KS - 1) - 1) / L.stride + 1;
    a.Wout = (Win + 2 * L.pad_w - L.dw * (L.KS - 1) - 1) / L.stride + 1;
    a.pad_h = L.pad_h; a.pad_w = L.pad_w;
}

// The batch statistics of a BatchNorm from the partial sums its producer left: `nparts` rows of `pstride` floats, `count` elements per channel.
static BNFinalizeArgs bn_finalize_args(const BN& b, const float* part, int nparts, int pstride, double count) {
    BNFinalizeArgs f{};
    f.part = part; f.nparts = nparts; f.pstride = pstride; f.count = count;
    f.w = b.w->dev; f.b = b.b->dev; f.rm = b.rm->dev; f.rv = b.rv->dev;
    f.affine = b.affine; f.save_mean = b.save_mean; f.save_invstd = b.save_invstd;
    f.C = b.C; f.eps = 1e-5f; f.momentum = 0.1f; f.broadcast = b.bcast;
    return f;
}

Tensor Model::run_conv(Conv& L, const std::vector<SrcSpec>& srcs_in, int N, const Tensor* out_view, const float* bias,
                       bool batch_as_h, FusedTail* tail) {
    // Training: give the conv plain inputs (one element-wise / upsample pass per source) -- the forward conv
    // then takes the LDS-DMA kernel and the weight gradient re-reads the same buffers without arithmetic.
    std::vector<SrcSpec> srcs = srcs_in;
    static const bool mat_enabled = !getenv("VR_NO_TRAIN_MAT");
    if (training && mat_enabled) {
        for (SrcSpec& sp : srcs) {
            const Tensor& t = sp.t;
            if (!(t.aff0 || t.aff1 || t.post || t.slope != 1.f || sp.up || sp.bcastH)) continue;
            const int vh = sp.up ? 2 * t.H : (sp.bcastH ? sp.bcastH : t.H), vw = sp.up ? 2 * t.W : t.W;
            float* buf = ws.allocf((size_t)t.N * t.C * vh * vw);
            if (!dry) {
                if (sp.up) launch_upsample2x(t, buf, stream);
                else {
                    Tensor v = t;
                    if (sp.bcastH) { v.H = sp.bcastH; v.sH = 0; }
                    launch_materialize(v, buf, stream);
                }
            }
            sp.plain = buf;
        }
    }
    ConvArgs a;
    build_fwd_args(L, srcs, N, batch_as_h, a);
    const ConvShape shp{L.KS, L.stride, L.dh, L.dw};
    if (!training) {
        // fused-upsample sources are for conv_x3.hip only: anything else gets the materialised tensor after all
        bool any_up = false;
        for (const SrcSpec& sp : srcs) any_up = any_up || sp.up;
        if (any_up) {
            ConvArgs probe = a;
            select_fwd_forms(probe, L.forms, form_select(), probe.Win, L.stride);
            probe.bf16 = mfma_mode;
            // ("the plan is conv_x3" is "x3_pick takes it" here: the 16-cout kernel ahead of it refuses any upsampled source)
            if (conv_plan(probe, shp).k != CK_X3) {
                for (SrcSpec& sp : srcs) {
                    if (!sp.up) continue;
                    const Tensor& t = sp.t;
                    Tensor u;
                    u.N = t.N; u.C = t.C; u.H = 2 * t.H; u.W = 2 * t.W;
                    u.sH = u.W; u.sC = (long long)u.H * u.W; u.sN = u.sC * u.C; u.slope = 1.f;
                    u.p = ws.allocf((size_t)u.N * u.C * u.H * u.W);
                    if (!dry) launch_upsample2x(t, u.p, stream);
                    sp = SrcSpec{u};
                }
                build_fwd_args(L, srcs, N, batch_as_h, a);
            }
        }
    }
    a.bias = bias;
    // Eval: the folded BatchNorm + activation go into the conv's epilogue, so the stored tensor is the
    // final activation and its consumers load it with no arithmetic (conv_dma.hip).  Training keeps
    // the raw tensor + pending affine: the batch statistics only exist after the whole conv has run.
    const bool fuse_epi = !training && L.bn != nullptr;
    if (fuse_epi) { a.epi = L.bn->affine; a.epi_slope = L.slope; }
    select_fwd_forms(a, L.forms, form_select(), a.Win, L.stride);
    a.bf16 = mfma_mode;
    int wcols = a.Wout;                                      // output columns the launch computes
    if (conv_w_hi > 0 && !training && mfma_mode == 3 && !batch_as_h && !conv_sink && conv_plan(a, shp).k == CK_X3) {
        a.w_lo = conv_w_lo; a.w_hi = conv_w_hi;                             // (the launch takes conv_x3h)
        wcols = std::min(a.Wout, (conv_w_hi + 31) / 32 * 32) - conv_w_lo / 32 * 32;
    }
    Tensor o;
    if (batch_as_h) {
        o.N = N; o.C = L.Cout; o.H = 1; o.W = a.Wout;
        if (out_view) { o.p = out_view->p; o.g = out_view->g; o.sN = out_view->sN; o.sC = out_view->sC; o.sH = out_view->sH; }
        else {
            o.p = ws.allocf((size_t)N * L.Cout * a.Wout); o.sN = (long long)L.Cout * a.Wout; o.sC = a.Wout; o.sH = a.Wout;
            if (taping()) o.g = galloc((size_t)N * L.Cout * a.Wout, false);      // (written through the batch-as-rows view: keep it zeroed)
        }
        a.dst[0] = ConvDst{o.p, 0, o.sC, o.sN, 0};
    } else {
        o.N = N; o.C = L.Cout; o.H = a.Hout; o.W = a.Wout;
        if (out_view) {
            VR_CHECK(out_view->H == a.Hout && out_view->W == a.Wout && out_view->C == L.Cout, -2, "conv " + L.name + ": output view shape mismatch");
            o.p = out_view->p; o.g = out_view->g; o.sN = out_view->sN; o.sC = out_view->sC; o.sH = out_view->sH;
        } else {
            o.p = ws.allocf((size_t)N * L.Cout * a.Hout * a.Wout);
            o.sH = a.Wout; o.sC = (long long)a.Hout * a.Wout; o.sN = o.sC * L.Cout;
            if (taping()) o.g = galloc((size_t)N * L.Cout * a.Hout * a.Wout, true);
        }
        a.dst[0] = ConvDst{o.p, o.sN, o.sC, o.sH, 0};
    }
    const bool stats = training && L.bn;
    BNFinalizeArgs fin{};
    if (stats) {
        const size_t npt = conv_part_count(a, shp);
        a.part = ws.allocf(npt * L.Cout * 2);
        fin = bn_finalize_args(*L.bn, a.part, (int)npt, L.Cout * 2, (double)N * (batch_as_h ? 1 : a.Hout) * a.Wout);
    }
    // The 1x1 stage that only reads this conv's output goes into the launch's epilogue where conv_x3h has the kernel for it (model.h:
    // FusedTail).  The workspace is laid out as without it (the dry run and every mode plan one sequence); a stage tail's producer
    // buffer is then simply not written.
    const char* fused_tag = "";
    if (tail && !dry && fuse_tail && !training && mfma_mode == 3 && !record_taps && !conv_sink && !batch_as_h && fuse_epi && a.w_hi == 0) {
        const ConvPlan plan = conv_plan(a, shp);
        if (plan.k == CK_X3) {                                             // (the launch takes conv_x3h)
            ConvArgs b = a;
            b.tail = tail->kind;
            b.t_p = tail->out.p;
            if (tail->kind == 1) {
                const Conv& L2 = *tail->L;
                VR_CHECK(L2.KS == 1 && L2.Cin == L.Cout && L2.bn && tail->out.C == L2.Cout && tail->out.H == a.Hout && tail->out.W == a.Wout, -3,
                         "fused stage tail: " + L2.name + " does not follow " + L.name);
                b.t_Cout = L2.Cout; b.t_CoutPad = L2.CoutPad; b.t_w = L2.w->dev; b.t_epi = L2.bn->affine; b.t_slope = L2.slope;
                b.t_sN = tail->out.sN; b.t_sC = tail->out.sC; b.t_sH = tail->out.sH;
            } else {
                const LSTMMod& M = *tail->M;
                VR_CHECK(M.squeeze.Cin == L.Cout, -3, "fused LSTM squeeze: " + M.squeeze.name + " does not follow " + L.name);
                b.t_Cout = 1; b.t_CoutPad = 1; b.t_w = M.squeeze.w->dev; b.t_epi = M.squeeze.bn->affine; b.t_slope = 0.f;
                b.t_sN = (long long)a.Hout * a.Wout; b.t_sC = 0; b.t_sH = a.Wout;
            }
            // Rule (profiles/fused_tail_ab.md): a site is fused where the one launch beats producer + consumer by at least half the consumer's
            // time at the 11-, 6- and 5-crop grids.  The squeeze behind the 64-cout dec2 with upsampled sources (stage 3) missed it at 6 crops
            // (13.6 us saved against a bar of 16.1; 23.9 / 22.9 at 11): it stays two launches.
            const bool any_up = a.src[0].up || (a.nsrc > 1 && a.src[1].up) || (a.nsrc > 2 && a.src[2].up);
            const bool by_rule = !(tail->kind == 2 && plan.MT == 64 && any_up);
            if (by_rule && x3h_tail_ok(b, plan)) {
                a = b;
                tail->done = true;
                fused_tag = tail->kind == 1 ? "+tail" : "+squeeze";
            }
        }
    }
    if (!dry && conv_sink) {
        // the caller launches this conv together with its siblings (ASPP branches: one conv_x3d launch for the four) and, in training,
        // finalises the BatchNorm statistics behind it
        PendingConv pc{};
        pc.a = a; pc.shp = shp;
        pc.flops = 2.0 * N * (double)a.Hout * a.Wout * (double)L.Cout * L.Cin * L.KS * L.KS;
        pc.bytes = conv_alg_bytes(L, a, N, batch_as_h);
        pc.stats = stats; pc.fin = fin; pc.bn = L.bn;
        conv_sink->push_back(pc);
    } else if (!dry) {
        const double flops = 2.0 * N * (double)(batch_as_h ? 1 : a.Hout) * wcols * (double)L.Cout * L.Cin * L.KS * L.KS;
        record_begin(0, flops);
        if (profiling) {
            // algorithmic HBM bytes of the launch: the virtual input, the 3x3/1x1 weights and the output, once each
            char tag[160];
            snprintf(tag, sizeof tag, "%s%s k%d s%d d%d ci%d co%d %dx%dx%d", L.name.c_str(), fused_tag, L.KS, L.stride, L.dh, L.Cin,
                     L.Cout, a.N, a.Hout, a.Wout);
            double bytes = conv_alg_bytes(L, a, N, batch_as_h);
            if (wcols < a.Wout) {                            // column window: the output and the full-resolution input over those columns (+ halo)
                const double fi = std::min(1.0, (wcols + 2.0) / a.Win), fo = (double)wcols / a.Wout;
                bytes = 4.0 * ((double)a.N * L.Cin * a.Hin * a.Win * fi + (double)N * L.Cout * a.Hout * a.Wout * fo +
                               (double)L.Cin * L.KS * L.KS * L.Cout);
                snprintf(tag + strlen(tag), sizeof tag - strlen(tag), " cols %d-%d", a.w_lo / 32 * 32, a.w_lo / 32 * 32 + wcols);
            }
            record_note(bytes, tag);
        }
        launch_conv(a, shp, stream);
        record_end();
        if (stats) {
            launch_bn_finalize(fin, stream);
            L.bn->nbt->nbt += 1;
        }
    }
    if (L.bn && !fuse_epi) { o.aff0 = L.bn->affine; o.slope = L.slope; } else { o.aff0 = nullptr; o.slope = 1.f; }
    if (taping()) {
        TapeRec r;
        r.kind = TK_CONV; r.L = &L; r.srcs = srcs; r.out = o; r.N = N; r.batch_as_h = batch_as_h; r.bias = bias;
        tape.push_back(std::move(r));
    }
    return o;
}

// layers.LSTMModule.forward (lib/layers.py:124-133)
Tensor Model::run_lstm(LSTMMod& M, const Tensor& h, float* z, bool squeezed) {
    const int N = h.N, nb = h.H, nf = h.W;
    VR_CHECK(nb == M.nin, -2, "LSTM input size does not match the number of bins at dec2");
    // 1x1 conv 2c -> 1 (+BN+ReLU): raw z [N][nb][nf] (the caller's buffer: dec2's launch may have filled it already, FusedTail)
    const int nblk = launch_squeeze_conv(h, M.squeeze.w->dev, z, nullptr, true, stream);
    float* part = training ? ws.allocf((size_t)nblk * 2) : nullptr;
    if (!dry && !squeezed) {
        // eval: BatchNorm (running statistics, folded) + ReLU in the kernel's store, so the LSTM input projection reads a plain tensor
        launch_squeeze_conv(h, M.squeeze.w->dev, z, part, false, stream, training ? nullptr : M.squeeze.bn->affine);
        if (training) {
            BN* b = M.squeeze.bn;
            launch_bn_finalize(bn_finalize_args(*b, part, nblk, 2, (double)N * nb * nf), stream);
            b->nbt->nbt += 1;
        }
    }
    // z as [N, C=nb, H=1, W=nf] (bins become channels): the LSTM input projection is a 1x1 conv
    Tensor zt;
    zt.p = z; zt.N = N; zt.C = nb; zt.H = 1; zt.W = nf;
    zt.sN = (long long)nb * nf; zt.sC = nf; zt.sH = nf;
    if (training) { zt.aff0 = M.squeeze.bn->affine; zt.slope = 0.f; }
    else zt.slope = 1.f;
    if (taping()) {
        zt.g = galloc((size_t)N * nb * nf, false);
        TapeRec r;
        r.kind = TK_SQUEEZE; r.M = &M; r.srcs = {SrcSpec{h}}; r.N = N;
        r.out = zt;                      // as a 1-channel image [N,1,nb,nf] for its own BatchNorm backward
        r.out.C = 1; r.out.H = nb; r.out.sC = (long long)nb * nf; r.out.sH = nf;
        tape.push_back(std::move(r));
    }
    const int G = 4 * M.hid;
    float* bias = ws.allocf((size_t)2 * G);               // (allocated in every mode: the planning dry run must see one sequence)
    if (!training && M.bias_sum) bias = M.bias_sum;       // eval: refreshed by fold_eval_affines()
    else if (!dry) {
        launch_add(M.b_ih_f->dev, M.b_hh_f->dev, bias, G, stream);
        launch_add(M.b_ih_r->dev, M.b_hh_r->dev, bias + G, G, stream);
    }
    // Eval (option "lstm_gemm", default 1): both matrix products of the module as rows_gemm.hip launches -- fp32 arithmetic, so in every
    // mfma_mode.  The workspace is laid out as run_conv lays it out (one buffer per product).
    const bool gemm = lstm_gemm && !training && !taping() && !conv_sink;
    auto rows_gemm = [&](Conv& L, const Tensor& x, const float* b) {
        Tensor o;
        o.N = N; o.C = L.Cout; o.H = 1; o.W = nf;
        o.p = ws.allocf((size_t)N * L.Cout * nf); o.sN = (long long)L.Cout * nf; o.sC = nf; o.sH = nf; o.slope = 1.f;
        if (dry) return o;
        RowsGemmArgs g{};
        g.x = x.p; g.xN = x.sN; g.w = L.w->dev; g.bias = b; g.out = o.p;
        if (L.bn) { g.epi = L.bn->affine; g.slope = L.slope; }
        g.N = N; g.T = nf; g.K = L.Cin; g.Cout = L.Cout; g.CoutPad = L.CoutPad;
        VR_CHECK(L.KS == 1 && x.C == L.Cin && x.sC == nf && rows_gemm_ok(g), -3, "rows_gemm: " + L.name + " is not a matrix product it takes");
        record_begin(0, 2.0 * N * (double)nf * L.Cout * L.Cin);
        if (profiling) {
            char tag[160];
            snprintf(tag, sizeof tag, "%s gemm ci%d co%d 1x%dx%d", L.name.c_str(), L.Cin, L.Cout, N, nf);
            record_note(4.0 * ((double)N * L.Cin * nf + (double)N * L.Cout * nf + (double)L.Cin * L.Cout), tag);
        }
        launch_rows_gemm(g, stream);
        record_end();
        return o;
    };
    Tensor gx = gemm ? rows_gemm(M.proj, zt, bias) : run_conv(M.proj, {SrcSpec{zt}}, N, nullptr, bias, true);       // [N][8H][nf]
    float* hc = ws.allocf((size_t)N * 2 * M.hid * nf);                          // [N][2H][nf]
    float* save = taping() ? ws.allocf((size_t)N * 2 * nf * 5 * M.hid) : nullptr;
    if (!dry) launch_bilstm_train(gx.p, M.whh_f->dev, M.whh_r->dev, hc, save, N, nf, M.hid, stream);
    Tensor ht;
    ht.p = hc; ht.N = N; ht.C = 2 * M.hid; ht.H = 1; ht.W = nf;
    ht.sN = (long long)2 * M.hid * nf; ht.sC = nf; ht.sH = nf; ht.slope = 1.f;
    if (taping()) {
        ht.g = galloc((size_t)N * 2 * M.hid * nf, false);
        TapeRec r;
        r.kind = TK_LSTM; r.M = &M; r.N = N; r.out = ht; r.aux = gx; r.save = save;
        tape.push_back(std::move(r));
    }
    Tensor lin = gemm ? rows_gemm(M.dense, ht, M.dense_b->dev) : run_conv(M.dense, {SrcSpec{ht}}, N, nullptr, M.dense_b->dev, true);   // [N][nb][nf] raw (eval: activated)
    if (taping()) tape.back().bias_param = M.dense_b;
    // BatchNorm1d + ReLU (lib/layers.py:120-121).  Eval: in place.  Train: the raw values are what the
    // BatchNorm backward needs, so the activated copy goes to its own buffer and shares lin's gradient.
    float* act = training ? ws.allocf((size_t)N * nb * nf) : lin.p;
    if (!dry && training) launch_rows_affine_relu(lin.p, act, M.dense.bn->affine, N, nb, nf, stream);   // eval: fused into the conv epilogue
    Tensor o;                                                                   // [N,1,nb,nf], already activated
    o.p = act; o.g = lin.g; o.N = N; o.C = 1; o.H = nb; o.W = nf;
    o.sN = (long long)nb * nf; o.sC = (long long)nb * nf; o.sH = nf; o.slope = 1.f;
    return o;
}

// Decoder input (lib/layers.py:52): training fuses the x2 bilinear upsample into the consuming conv's
// loader; eval materialises it once (HBM-bound, small) so the conv reads a plain tensor by LDS-DMA.
Model::SrcSpec Model::upsampled(const Tensor& t) {
    if (training) {
        SrcSpec s{t};
        s.up = true;
        return s;
    }
    // Eval, split-bf16 mode: conv_x3.hip interpolates while it splits the pixels into bf16 planes, so the full-resolution decoder
    // layers read the LOW-resolution tensor (a quarter of the bytes) and nothing is materialised.  Measured per layer (tools/
    // x3_proto.hip): it pays from 512 x 128 output pixels on (dec1, stage-3 dec2); below, the interpolation VALU of the many-channel
    // layers costs more than the HBM-bound upsample pass.
    static const bool fuse_on = !(getenv("VR_X3_FUSE_UP") && atoi(getenv("VR_X3_FUSE_UP")) == 0);
    static const bool x3_on = !(getenv("VR_CONV_X3") && atoi(getenv("VR_CONV_X3")) == 0);
    if (fuse_on && x3_on && x3_mode() && 4LL * t.H * t.W >= 65536 && 2 * t.W >= 32 && !t.aff0 && !t.aff1 && !t.post && t.slope == 1.f) {
        SrcSpec s{t};
        s.up = true;
        return s;
    }
    Tensor u;
    u.N = t.N; u.C = t.C; u.H = 2 * t.H; u.W = 2 * t.W;
    u.sH = u.W; u.sC = (long long)u.H * u.W; u.sN = u.sC * u.C; u.slope = 1.f;
    u.p = ws.allocf((size_t)u.N * u.C * u.H * u.W);
    if (!dry) launch_upsample2x(t, u.p, stream);
    return SrcSpec{u};
}

// nets.BaseNet.__call__ (lib/nets.py:26-41)
Tensor Model::run_basenet(BaseNetL& B, const std::vector<SrcSpec>& in, int N, const Tensor* out_view, FusedTail* tail) {
    const std::string& p = B.prefix;
    Tensor e[5];
    e[0] = run_conv(B.enc1, in, N, nullptr, nullptr, false);
    tap(p + ".e1", e[0]);
    for (int i = 0; i < 4; ++i) {
        Tensor t = run_conv(B.enc_a[i], {SrcSpec{e[i]}}, N, nullptr, nullptr, false);
        e[i + 1] = run_conv(B.enc_b[i], {SrcSpec{t}}, N, nullptr, nullptr, false);
        tap(p + ".e" + std::to_string(i + 2), e[i + 1]);
    }
    // layers.ASPPModule.forward (lib/layers.py:92-105)
    const Tensor& x5 = e[4];
    const int C8 = 8 * B.c;
    float* pooled = ws.allocf((size_t)N * C8 * x5.W);
    // Eval, mfma_mode 3 (round 6): the four branch convs go out as ONE launch on the fp16 matrix pipe (conv_x3d.hip: blockIdx.y = branch).
    // They are collected first; if any of them does not qualify (another mode, VR_ASPP_FUSED=0) each is launched on its own as before.
    const bool group = !dry && mfma_mode == 3 && x3d_mode == 2 && !(training && !train_wino);
    // Eval (option "aspp_pool_fused", default 1): the pooled branch -- the mean over H and conv1.1 -- waits for that launch too and rides in
    // it as a fifth part (X3dPoolArgs) where the launch can carry it; where not, its two launches go out in front of the group's.
    const bool pool_wait = group && !training && aspp_pool_fused;
    if (!dry && !pool_wait) launch_avgpool_h(x5, pooled, stream);
    Tensor pt;
    pt.p = pooled; pt.N = N; pt.C = C8; pt.H = 1; pt.W = x5.W;
    pt.sN = (long long)C8 * x5.W; pt.sC = x5.W; pt.sH = x5.W; pt.slope = 1.f;
    if (taping()) {
        pt.g = galloc((size_t)N * C8 * x5.W, false);
        TapeRec r;
        r.kind = TK_AVGPOOL; r.srcs = {SrcSpec{x5}}; r.out = pt; r.N = N;
        tape.push_back(std::move(r));
    }
    std::vector<PendingConv> pend_pool;
    if (pool_wait) conv_sink = &pend_pool;
    Tensor f1;
    try { f1 = run_conv(B.aspp_pool, {SrcSpec{pt}}, N, nullptr, nullptr, true); } catch (...) { conv_sink = nullptr; throw; }
    conv_sink = nullptr;
    // conv2..conv5 write channel slices of one [N, 4*C8, H, W] buffer (the concat is never built)
    Tensor cat4;
    cat4.N = N; cat4.C = 4 * C8; cat4.H = x5.H; cat4.W = x5.W;
    cat4.sH = x5.W; cat4.sC = (long long)x5.H * x5.W; cat4.sN = cat4.sC * cat4.C;
    cat4.p = ws.allocf((size_t)N * cat4.C * x5.H * x5.W);
    if (taping()) cat4.g = galloc((size_t)N * cat4.C * x5.H * x5.W, false);
    if (training) { cat4.aff0 = B.aspp_aff; cat4.slope = 0.f; }      // eval: the branch convs store final activations
    Conv* branch[4] = {&B.aspp_c2, &B.aspp_d[0], &B.aspp_d[1], &B.aspp_d[2]};
    // Training: the four branches read the same activated tensor -- materialised ONCE here (run_conv would do it once per branch); the plain
    // copy shares x5's gradient buffer, so the four data gradients still meet in x5.g
    Tensor x5b = x5;
    {
        static const bool mat_enabled = !getenv("VR_NO_TRAIN_MAT");
        if (training && mat_enabled && (x5.aff0 || x5.aff1 || x5.post || x5.slope != 1.f)) {
            float* buf = ws.allocf((size_t)N * C8 * x5.H * x5.W);
            if (!dry) launch_materialize(x5, buf, stream);
            x5b.p = buf; x5b.aff0 = x5b.aff1 = nullptr; x5b.post = nullptr; x5b.slope = 1.f; x5b.hsplit = 1 << 30;
            x5b.sH = x5.W; x5b.sC = (long long)x5.H * x5.W; x5b.sN = x5b.sC * C8;
        }
    }
    // Eval, stage 3: the four branch convs are independent and each fills < 256 CUs at 1/16 resolution --
    // two of them go to the idle side stream.
    static const bool aspp_fork = !getenv("VR_NO_ASPP_FORK");
    std::vector<PendingConv> pend;
    const bool afk = aspp_fork && !serial && !training && !dry && !profiling && side_stream != nullptr && !band_fork_active && !group;
    hipStream_t aspp_main = stream;
    // (Round 5, measured and removed: every branch on its own stream -- three auxiliary streams per lane, in every stage -- made the
    // inference step 12.4 ms instead of 8.65, also with 8 or 16 hardware queues: each extra fork / join pair costs more than the overlap
    // of four ~60 us kernels returns.  Two streams, stage 3 only, is the measured optimum.)
    if (afk) {
        hipEvent_t ef = ev_fork;
        VR_HIP(hipEventRecord(ef, aspp_main));
        VR_HIP(hipStreamWaitEvent(side_stream, ef, 0));
    }
    for (int j = 0; j < 4; ++j) {
        Tensor v = cat4;
        v.C = C8;
        v.p = dry ? cat4.p : cat4.p + (long long)j * C8 * cat4.sC;
        if (taping() && !dry) v.g = cat4.g + (long long)j * C8 * cat4.sC;
        if (afk) stream = (j & 1) ? side_stream : aspp_main;
        if (group) conv_sink = &pend;
        try { run_conv(*branch[j], {SrcSpec{x5b}}, N, &v, nullptr, false); } catch (...) { stream = aspp_main; conv_sink = nullptr; throw; }
        conv_sink = nullptr;
    }
    if (group) {
        VR_CHECK(pend.size() == 4, -3, "ASPP: four branch convs expected");
        ConvArgs c4[4];
        ConvShape s4[4];
        double flops = 0.0, bytes = 0.0;
        for (int j = 0; j < 4; ++j) { c4[j] = pend[j].a; s4[j] = pend[j].shp; flops += pend[j].flops; bytes += pend[j].bytes; }
        const bool grouped = x3d_aspp_eligible(c4, s4);
        X3dPoolArgs q{};
        if (pool_wait) {
            VR_CHECK(pend_pool.size() == 1, -3, "ASPP: the pooled branch's conv expected");
            const ConvArgs& pa = pend_pool[0].a;
            const ConvSrc& xs = c4[0].src[0];                    // x5 as the branch convs read it (x3d_pick: one plain source)
            q.x = xs.p; q.xN = xs.sN; q.xC = xs.sC; q.xH = xs.sH;
            q.w = pa.w; q.epi = pa.epi; q.slope = pa.epi ? pa.epi_slope : 1.f; q.out = f1.p;
            q.C8 = C8; q.H = x5.H; q.Cout = pa.Cout; q.CoutPad = pa.CoutPad;
        }
        const bool pool_in = pool_wait && grouped && c4[0].nsrc == 1 && !pend_pool[0].a.bias && f1.sN == (long long)q.Cout * 16 && f1.sC == 16 &&
                             x3d_pool_eligible(q, c4);
        if (pool_wait && !pool_in) {
            launch_avgpool_h(x5, pooled, stream);
            record_begin(0, pend_pool[0].flops);
            if (profiling) record_note(pend_pool[0].bytes, B.aspp_pool.name.c_str());
            launch_conv(pend_pool[0].a, pend_pool[0].shp, stream);
            record_end();
        }
        if (grouped) {
            // the pooled part's own work: the mean reads x5 (counted with the branches) and 1x1 weights, and writes f1
            const double pflops = pool_in ? (double)N * C8 * x5.H * x5.W + pend_pool[0].flops : 0.0;
            const double pbytes = pool_in ? 4.0 * ((double)C8 * C8 + (double)N * C8 * x5.W) : 0.0;
            record_begin(0, flops + pflops);
            if (profiling) {
                char tag[160];
                snprintf(tag, sizeof tag, "%s.aspp.conv2-5%s k1+3x(k3 d4/8/12) ci%d co%d %dx%dx%d", p.c_str(), pool_in ? "+pool+conv1" : "", C8, C8, N,
                         x5.H, x5.W);
                // (the four read the same input: counted once)
                record_note(bytes - 3.0 * 4.0 * (double)N * C8 * x5.H * x5.W + pbytes, tag);
            }
            x3d_launch_aspp(c4, stream, pool_in ? &q : nullptr);
            record_end();
        } else {
            for (int j = 0; j < 4; ++j) {
                record_begin(0, pend[j].flops);
                if (profiling) record_note(pend[j].bytes, branch[j]->name.c_str());
                launch_conv(c4[j], s4[j], stream);
                record_end();
            }
        }
        for (int j = 0; j < 4; ++j)
            if (pend[j].stats) {
                launch_bn_finalize(pend[j].fin, stream);
                pend[j].bn->nbt->nbt += 1;
            }
    }
    if (afk) {
        stream = aspp_main;
        hipEvent_t ej = ev_join;
        VR_HIP(hipEventRecord(ej, side_stream));
        VR_HIP(hipStreamWaitEvent(aspp_main, ej, 0));
    }
    SrcSpec s1{f1};
    s1.bcastH = x5.H;          // bilinear from H=1 with align_corners=True is a broadcast along H
    Tensor h = run_conv(B.aspp_bott, {s1, SrcSpec{cat4}}, N, nullptr, nullptr, false);
    if (training && dropout_dev) {
        int idx = (int)(&B - nets_);
        h.post = dropout_dev + (size_t)idx * N * 8 * nout;   // [5][N][8*nout] slots, row pitch 8c
        if (taping()) tape.back().out.post = h.post;          // the bottleneck's BatchNorm backward needs it
    }
    tap(p + ".aspp", h);
    // decoders (lib/layers.py:51-64): upsample x2 + skip concat + conv, all inside the conv's loader
    // (the LSTM squeeze reads only dec2's output: its buffer exists before dec2 runs, so that dec2's launch can fill it, FusedTail)
    FusedTail sq;
    sq.kind = 2; sq.M = &B.lstm;
    for (int i = 0; i < 3; ++i) {
        SrcSpec up = upsampled(h);
        if (i == 2) sq.out.p = ws.allocf((size_t)N * e[1].H * e[1].W);
        h = run_conv(B.dec[i], {up, SrcSpec{e[3 - i]}}, N, nullptr, nullptr, false, i == 2 ? &sq : nullptr);
        tap(p + ".dec" + std::to_string(4 - i), h);
    }
    // Eval, stage 3 (the side stream is idle there): the x2 upsample of h (HBM-bound) runs beside the LSTM branch
    // (latency-bound); both only need h, and dec1 needs both.
    static const bool lstm_fork = !getenv("VR_NO_LSTM_FORK");
    const bool fk = lstm_fork && !serial && !training && !dry && !profiling && side_stream != nullptr && !band_fork_active;
    SrcSpec uh;
    hipEvent_t lstm_join = nullptr;
    if (fk) {
        hipStream_t ms = stream;
        hipEvent_t ef = ev_fork;
        VR_HIP(hipEventRecord(ef, ms));
        VR_HIP(hipStreamWaitEvent(side_stream, ef, 0));
        stream = side_stream;
        try { uh = upsampled(h); } catch (...) { stream = ms; throw; }
        lstm_join = ev_join;
        VR_HIP(hipEventRecord(lstm_join, side_stream));
        stream = ms;
    }
    Tensor l = run_lstm(B.lstm, h, sq.out.p, sq.done);
    tap(p + ".lstm", l);
    if (fk) VR_HIP(hipStreamWaitEvent(stream, lstm_join, 0));
    else uh = upsampled(h);
    SrcSpec ul = upsampled(l);
    // (stage 3 under a caller's column window: only the head reads this output, and only those columns)
    const bool win = &B == &nets_[4] && net_w_hi > 0;
    if (win) { conv_w_lo = net_w_lo; conv_w_hi = net_w_hi; }
    Tensor o;
    try { o = run_conv(B.dec[3], {uh, ul, SrcSpec{e[0]}}, N, out_view, nullptr, false, tail); } catch (...) { conv_w_lo = conv_w_hi = 0; throw; }
    conv_w_lo = conv_w_hi = 0;
    tap(p + ".dec1", o);
    return o;
}

// CascadedNet.forward up to (not including) `out` (lib/nets.py:86-102)
Tensor Model::run_net(const Tensor& x) {
    const int B = x.N, T = x.W;
    const int bandw = max_bin / 2;
    Tensor xl = x; xl.H = bandw;
    Tensor xh = x; xh.H = bandw; xh.p = dry ? x.p : x.p + (long long)bandw * x.sH;
    auto make_aux = [&](int C) {
        Tensor t;
        t.N = B; t.C = C; t.H = max_bin; t.W = T;
        t.sH = T; t.sC = (long long)max_bin * T; t.sN = t.sC * C;
        t.p = ws.allocf((size_t)B * C * max_bin * T);
        if (taping()) t.g = galloc((size_t)B * C * max_bin * T, false);          // written through the full view and the band halves
        t.slope = training ? 0.f : 1.f;     // eval: dec1 / the tail convs store final activations
        return t;
    };
    Tensor aux1 = make_aux(nout / 4), aux2 = make_aux(nout / 2);
    auto half = [&](const Tensor& a, int which) {
        Tensor v = a; v.H = bandw;
        if (which && !dry) { v.p = a.p + (long long)bandw * a.sH; if (a.g) v.g = a.g + (long long)bandw * a.sH; }
        return v;
    };
    Tensor v;
    // The low-band chain (stg1_low -> stg2_low) and the high-band chain (stg1_high -> stg2_high) are
    // independent until stage 3 (lib/nets.py:91-98).  They run on two HIP streams (forward of both modes) so the
    // small 1/16-resolution layers of one chain fill the CUs the other leaves idle.
    // (not while per-kernel HIP-event timing is on: overlapping kernels would inflate each other's time)
    static const bool train_fork = !getenv("VR_NO_TRAIN_FORK");
    static const bool band_fork = !getenv("VR_NO_BAND_FORK");
    const bool fork = band_fork && !serial && !dry && (!training || train_fork) && !profiling && side_stream != nullptr;
    hipStream_t main_stream = stream;
    if (fork) {
        hipEvent_t ef = ev_fork;
        VR_HIP(hipEventRecord(ef, main_stream));
        VR_HIP(hipStreamWaitEvent(side_stream, ef, 0));
        band_fork_active = true;                 // until the join: the side stream belongs to the high-band chain
    }
    // the low-band nets end in a 1x1 Conv2DBNActiv that is dec1's only reader: offered to dec1's launch (FusedTail); what that launch
    // has stored is the tail's output -- the tensor run_conv(tail) returns in eval: final activations, no pending affine
    auto low_band = [&](BaseNetL& net, Conv& tl, const std::vector<SrcSpec>& in, const Tensor& view) {
        FusedTail ft;
        ft.kind = 1; ft.L = &tl; ft.out = view; ft.out.C = tl.Cout;
        Tensor r = run_basenet(net, in, B, nullptr, &ft);
        if (!ft.done) return run_conv(tl, {SrcSpec{r}}, B, &view, nullptr, false);
        Tensor o;
        o.N = B; o.C = tl.Cout; o.H = view.H; o.W = view.W;
        o.p = view.p; o.g = view.g; o.sN = view.sN; o.sC = view.sC; o.sH = view.sH;
        o.aff0 = nullptr; o.slope = 1.f;
        return o;
    };
    v = half(aux1, 0);
    Tensor l1 = low_band(nets_[0], tail1, {SrcSpec{xl}}, v);
    v = half(aux2, 0);
    Tensor l2 = low_band(nets_[2], tail2, {SrcSpec{xl}, SrcSpec{l1}}, v);
    if (fork) stream = side_stream;
    const size_t tape_hi0 = tape.size();
    v = half(aux1, 1);
    Tensor h1 = run_basenet(nets_[1], {SrcSpec{xh}}, B, &v);
    v = half(aux2, 1);
    Tensor h2 = run_basenet(nets_[3], {SrcSpec{xh}, SrcSpec{h1}}, B, &v);
    for (size_t i = tape_hi0; i < tape.size(); ++i) tape[i].chain = 1;    // backward may run these beside the low chain
    if (fork) {
        hipEvent_t ej = ev_join;
        VR_HIP(hipEventRecord(ej, side_stream));
        stream = main_stream;
        VR_HIP(hipStreamWaitEvent(main_stream, ej, 0));
        band_fork_active = false;
    }
    tap("l1", l1); tap("h1", h1);
    tap("l2", l2); tap("h2", h2);
    aux1.aff0 = l1.aff0; aux1.aff1 = h1.aff0; aux1.hsplit = bandw;
    aux2.aff0 = l2.aff0; aux2.aff1 = h2.aff0; aux2.hsplit = bandw;
    Tensor xf = x; xf.H = max_bin;
    Tensor f3 = run_basenet(nets_[4], {SrcSpec{xf}, SrcSpec{aux1}, SrcSpec{aux2}}, B, nullptr);
    return f3;
}

// run_net for a caller that keeps only the mask columns [w_lo, w_hi) (w_hi == 0: all): with "crop_window" on, in eval and mfma_mode 3
// and while no taps are recorded (the parity tests compare every dec1 tap at full width), stage 3's dec1 computes only those columns
Tensor Model::run_net_window(const Tensor& x, int w_lo, int w_hi) {
    if (!(crop_window && !training && mfma_mode == 3 && !record_taps && w_hi > 0 && w_lo > 0)) return run_net(x);
    net_w_lo = w_lo; net_w_hi = w_hi;
    Tensor f3;
    try { f3 = run_net(x); } catch (...) { net_w_lo = net_w_hi = 0; throw; }
    net_w_lo = net_w_hi = 0;
    return f3;
}

void Model::plan_and_reserve(int B, int T, size_t extra_bytes) {
    graph_valid = false;                         // the workspace is about to be rewound: a kept training graph dies here
    // the dry run is pure host work (~0.3 ms for the full net): remember its result per (B, T, mode)
    if (plan_B == B && plan_T == T && plan_training == training && plan_peak > 0) {
        ensure_ws(plan_peak + extra_bytes + 4096);
        ws.reset();
        return;
    }
    Arena saved = ws;
    ws.dry = true; ws.base = nullptr; ws.off = 0; ws.peak = 0;
    dry = true;
    Tensor x;
    x.p = reinterpret_cast<float*>(uintptr_t(256));
    x.N = B; x.C = nin; x.H = max_bin; x.W = T; x.sH = T; x.sC = (long long)output_bin * T; x.sN = nin * x.sC;
    try { run_net(x); } catch (...) { dry = false; ws = saved; throw; }
    dry = false;
    const size_t need = ws.peak + extra_bytes + 4096;
    plan_B = B; plan_T = T; plan_training = training; plan_peak = ws.peak;
    ws = saved;
    ensure_ws(need);
    ws.reset();
}

static void check_T(int T, int offset, int mode) {
    VR_CHECK(T > 0 && T % 16 == 0, -5, "h1_shape[3] must be greater than h2_shape[3] (frames must be a multiple of 16)");
    if (mode != 0) VR_CHECK(T - 2 * offset > 0, -6, "assert mask.size()[3] > 0 (frames must exceed 2*offset)");
}

// m *= x[.., off + w]; CPLX: complex64 x and m, the complex product (predict of a complex handle); `total` counts elements
template <bool CPLX>
__global__ void mul_crop_kernel(const float* __restrict__ x, float* __restrict__ m, int T, int Wm, int off, long long total) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int w = (int)(gid % Wm);
    const long long row = gid / Wm;
    if constexpr (CPLX) {
        const float2 a = reinterpret_cast<const float2*>(x)[row * T + off + w];
        float2* mc = reinterpret_cast<float2*>(m) + gid;
        const float2 b = *mc;
        *mc = make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
    } else {
        m[gid] *= x[row * T + off + w];
    }
}

void launch_mul_crop(const float* x, float* m, bool cplx, long long rows, int T, int Wm, int off, hipStream_t st) {
    const long long total = rows * Wm;
    if (cplx) VR_LAUNCH((mul_crop_kernel<true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, m, T, Wm, off, total);
    else VR_LAUNCH((mul_crop_kernel<false>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, m, T, Wm, off, total);
    VR_HIP(hipGetLastError());
}

// The network's input from X [B][2][bins][T] (complex handle: complex64).  copy given: X (on the host or the device, as *copy says) goes
// into a workspace copy first; *xd (if asked) is where X then lies on the device.  A complex handle's input is packed into the planar
// [B][4][bins][T] (re L, re R, im L, im R: the reference's cat([x.real, x.imag])), unscaled.  dry: sizes only.
Tensor Model::net_input(const float* X, const hipMemcpyKind* copy, int B, int T, const float** xd) {
    const size_t planes = (size_t)B * 2 * output_bin * T;
    if (copy) {
        float* c = ws.allocf(planes * (is_complex ? 2 : 1));
        VR_HIP(hipMemcpyAsync(c, X, planes * (is_complex ? 2 : 1) * sizeof(float), *copy, stream));
        X = c;
    }
    if (xd) *xd = X;
    Tensor xt;
    xt.p = const_cast<float*>(X); xt.N = B; xt.C = nin; xt.H = max_bin; xt.W = T;
    xt.sH = T; xt.sC = (long long)output_bin * T; xt.sN = nin * xt.sC; xt.slope = 1.f;
    if (is_complex) {
        xt.p = ws.allocf(2 * planes);
        if (!dry) launch_pack_complex(reinterpret_cast<const float2*>(X), B, output_bin, T, xt.p, T, 0, nullptr, stream);
    }
    return xt;
}

// the mask head of this handle's kind (sigmoid or complex) over the columns [w_lo, w_hi) of f3, dense [B][2][bins][w_hi - w_lo] at `out`
void Model::mask_head(const Tensor& f3, int w_lo, int w_hi, float* out) {
    HeadDst d{};
    d.p = out; d.dH = w_hi - w_lo; d.dC = (long long)output_bin * d.dH; d.dN = 2 * d.dC;       // (complex handle: complex elements)
    mask_head(f3, w_lo, w_hi, d);
}

void Model::forward_api(const float* x, bool x_on_device, int B, int T, int mode, float* out, bool out_on_device) {
    DeviceGuard dev_guard(device);
    VR_CHECK(B > 0, -2, "batch must be positive");
    check_T(T, offset, mode);
    if (is_complex) need_real_mask_train("vr_forward");
    const size_t E = is_complex ? 2 : 1;             // floats per element: a complex handle takes and gives complex64
    const size_t in_floats = (size_t)B * 2 * output_bin * T * E;
    const size_t pack_floats = is_complex ? (size_t)B * 4 * output_bin * T : 0;
    const int Wm = mode == 0 ? T : T - 2 * offset;
    const size_t out_floats = (size_t)B * 2 * output_bin * Wm * E;
    // Train mode (the reference's `model(X)` under model.train(), train.py:81 without the backward): BatchNorm uses
    // and updates batch statistics, Dropout2d is live, but no tape and no gradient buffers are kept.
    struct FwdOnly { Model* m; ~FwdOnly() { m->fwd_only = false; m->dropout_dev = nullptr; } } fwd_scope{this};
    fwd_only = training;
    if (training) refresh_forms(false);     // before planning: the kernel choice (and its partial-statistics layout) depends on them
    if (!training) fold_eval_affines();     // (eval: the bf16-plane weight tables decide conv_x3 vs the materialised-upsample plan)
    plan_and_reserve(B, T, (in_floats + pack_floats + out_floats) * sizeof(float) + 1024 * E);
    if (training) prepare_dropout(B);
    const hipMemcpyKind kind = x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float* xd = nullptr;
    const Tensor xt = net_input(x, &kind, B, T, &xd);
    float* od = out_on_device ? out : ws.allocf(out_floats);
    if (record_taps) taps.clear();
    Tensor f3 = run_net_window(xt, mode == 0 ? 0 : offset, mode == 0 ? 0 : T - offset);
    mask_head(f3, mode == 0 ? 0 : offset, mode == 0 ? T : T - offset, od);
    if (mode == 2) launch_mul_crop(xd, od, is_complex, (long long)B * 2 * output_bin, T, Wm, offset, stream);
    if (!out_on_device) VR_HIP(hipMemcpyAsync(out, od, out_floats * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    if (training) affine_dirty = true;
}

// sum |pred - crop_center(y)| per block; pred [rows][Wm] dense, y [rows][T] dense, columns [off, off+Wm) of y
// CPLX: complex64 pred and y, |.| of the complex difference (torch's L1Loss on complex tensors); `total` counts elements
// MODE (at most one type; a trailing pack keeps the names of the forms above): MagL1 (CPLX only) = | |pred| - |y| |, the magnitude part of
// VR_LOSS_MAG_L1_WAVE_SDR
template <bool CPLX, class... MODE>
__global__ __launch_bounds__(256) void l1_crop_kernel(const float* __restrict__ pred, const float* __restrict__ y, int T, int Wm,
                                                      int off, long long total, float* __restrict__ part) {
    constexpr bool kMag = sizeof...(MODE) == 1;
    static_assert(sizeof...(MODE) <= 1 && (!kMag || CPLX), "one mode at most; the magnitude form takes complex input");
    float s = 0.f;
    for (long long gid = (long long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long long)gridDim.x * 256) {
        const int w = (int)(gid % Wm);
        const long long row = gid / Wm;
        if constexpr (CPLX) {
            const float2 a = reinterpret_cast<const float2*>(pred)[gid], b = reinterpret_cast<const float2*>(y)[row * T + off + w];
            if constexpr (kMag) s += fabsf(hypotf(b.x, b.y) - hypotf(a.x, a.y));
            else s += hypotf(a.x - b.x, a.y - b.y);
        } else {
            s += fabsf(pred[gid] - y[row * T + off + w]);
        }
    }
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

int l1_crop_blocks() { return 1024; }

void launch_l1_crop(L1CropForm form, const float* pred, const float* y, long long rows, int T, int Wm, int off, float* part, float* loss,
                    hipStream_t st) {
    const long long total = rows * Wm;
    const int nblk = l1_crop_blocks();
    if (form == L1_CROP_REAL) VR_LAUNCH((l1_crop_kernel<false>), dim3(nblk), dim3(256), 0, st, pred, y, T, Wm, off, total, part);
    else if (form == L1_CROP_COMPLEX) VR_LAUNCH((l1_crop_kernel<true>), dim3(nblk), dim3(256), 0, st, pred, y, T, Wm, off, total, part);
    else VR_LAUNCH((l1_crop_kernel<true, MagL1>), dim3(nblk), dim3(256), 0, st, pred, y, T, Wm, off, total, part);
    VR_HIP(hipGetLastError());
    launch_reduce_rows(part, 1, nblk, loss, 1, 0, (float)(1.0 / (double)total), st);
}

// vr_set_loss: which loss vr_train_step / vr_validate_step compute on this handle.  Every refusal comes before the
// device is touched.
void Model::set_loss(int kind, double weight) {
    VR_CHECK(kind == 0 || kind == 1 || kind == 3, -2,
             "vr_set_loss: kind must be VR_LOSS_L1 (0), VR_LOSS_MAG_L1_WAVE_SDR (1) or VR_LOSS_MAG_L1_WAVE_WSDR (3)");
    if (kind != 0) {
        const std::string name = kind == 3 ? "VR_LOSS_MAG_L1_WAVE_WSDR" : "VR_LOSS_MAG_L1_WAVE_SDR";
        VR_CHECK(is_complex, -2, "vr_set_loss: " + name + " needs a complex-mask handle (VR_CREATE_COMPLEX): the inverse STFT of "
                                 "its wave term takes a complex spectrogram, and this handle predicts a magnitude mask");
        VR_CHECK(complex_train, -2, "vr_set_loss: " + name + " needs the option complex_train on (vr_set_option(h, \"complex_train\", 1)): "
                                    "the training entry points refuse this complex handle without it");
        VR_CHECK(wave_loss_available(plan, hop), -2, "vr_set_loss: " + name + " needs hop_length == n_fft / 2 (128 <= n_fft <= 4096), the "
                                                     "tiled signal path; this handle has n_fft " + std::to_string(n_fft) + ", hop " + std::to_string(hop));
        VR_CHECK(std::isfinite(weight), -2, "vr_set_loss: sdr_weight must be finite");
    }
    loss_kind = kind;
    sdr_weight = kind != 0 ? weight : 0.01;
    last_mag_l1 = last_sdr = last_y_sdr = last_noise_sdr = last_alpha = 0.0;
    loss_terms_valid = false;
    graph_valid = false;
}

// lossd [4] = (mean | |y| - |p| |, <y, p>, <y, y>, <p, p>) -> the two terms and the loss, combined in double
float Model::finish_wave_loss(const float* l4) {
    const double D = std::sqrt((double)l4[2]) * std::sqrt((double)l4[3]) + 1e-8;
    last_mag_l1 = (double)l4[0];
    last_sdr = -(double)l4[1] / D;
    loss_terms_valid = true;
    return (float)(last_mag_l1 + sdr_weight * last_sdr);
}

// lossd [7] = (mean | |y| - |p| |, <y, p>, <y, y>, <p, p>, <n, q>, <n, n>, <q, q>) -> the terms of VR_LOSS_MAG_L1_WAVE_WSDR and the
// loss, combined in double as the reference's weighted_sdr_loss combines them (train.py:53-65)
float Model::finish_wsdr_loss(const float* l7) {
    const double A1 = l7[1], yy = l7[2], pp = l7[3], A2 = l7[4], nn = l7[5], qq = l7[6], eps = 1e-8;
    last_mag_l1 = (double)l7[0];
    last_y_sdr = A1 / (std::sqrt(yy) * std::sqrt(pp) + eps);
    last_noise_sdr = A2 / (std::sqrt(nn) * std::sqrt(qq) + eps);
    last_alpha = yy / (yy + nn + eps);
    last_sdr = -(last_alpha * last_y_sdr + (1.0 - last_alpha) * last_noise_sdr);
    loss_terms_valid = true;
    return (float)(last_mag_l1 + sdr_weight * last_sdr);
}

// One batch of train.validate_epoch (train.py:117-127): y_pred = model.predict(X); y = crop_center(y, y_pred);
// loss = L1Loss()(y_pred, y) -- forward, crop and the mean-absolute-error reduction all on the device.
void Model::validate_api(const float* X, const float* Y, bool on_dev, int B, int T, float* loss_out) {
    DeviceGuard dev_guard(device);
    need_real_mask("vr_validate_step (its L1 loss is defined on magnitudes)");
    VR_CHECK(!training, -2, "validate step runs in eval mode (train.py:109 model.eval()); call vr_set_mode(h, 0) first");
    VR_CHECK(B > 0, -2, "batch must be positive");
    check_T(T, offset, 2);                           // T % 16 == 0 and T > 2 * offset: the cropped width Wm is at least 16 frames
    const size_t E = is_complex ? 2 : 1;             // floats per element: a complex handle takes and predicts complex64
    const size_t in_floats = (size_t)B * 2 * output_bin * T * E;
    const size_t pack_floats = is_complex ? (size_t)B * 4 * output_bin * T : 0;
    const int Wm = T - 2 * offset;
    const size_t out_floats = (size_t)B * 2 * output_bin * Wm * E;
    const int nblk = l1_crop_blocks();
    // VR_LOSS_MAG_L1_WAVE_SDR: both waves of the cropped pair and the pair kernel's partial sums
    // VR_LOSS_MAG_L1_WAVE_WSDR: the mixture's wave too, and six partial sums per workgroup
    const bool wsdr_loss = loss_kind == 3, wave_loss = loss_kind == 1 || wsdr_loss;
    const int signals = B * 2;
    const WaveTermFloats wf = wave_loss ? wave_term_floats(plan, hop, loss_kind, signals, Wm) : WaveTermFloats{};
    const size_t loss_extra = wave_loss ? wf.waves * wf.wave + wf.part + 256 : 0;
    fold_eval_affines();                    // before planning, as in forward_api
    plan_and_reserve(B, T, (2 * in_floats + pack_floats + out_floats + nblk + 64 + loss_extra) * sizeof(float) + 8192);
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float *xd = nullptr, *yd = Y;
    const Tensor xt = net_input(X, &kind, B, T, &xd);
    if (!on_dev) {
        float* ty = ws.allocf(in_floats);
        VR_HIP(hipMemcpyAsync(ty, Y, in_floats * sizeof(float), hipMemcpyHostToDevice, stream));
        yd = ty;
    }
    float* od = ws.allocf(out_floats);
    float* part = ws.allocf(nblk);
    float* lossd = ws.allocf(16);
    Tensor f3 = run_net_window(xt, offset, T - offset);
    const long long rows = (long long)B * 2 * output_bin;
    float l4[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // p = predict(X) as materialised, then the loss of the handle's kind on p and crop_center(y)
    mask_head(f3, offset, T - offset, od);
    launch_mul_crop(xd, od, is_complex, rows, T, Wm, offset, stream);
    if (wave_loss) prof_memset_async(lossd, 0, (wsdr_loss ? 7 : 4) * sizeof(float), stream);
    launch_l1_crop(wave_loss ? L1_CROP_MAG : is_complex ? L1_CROP_COMPLEX : L1_CROP_REAL, od, yd, rows, T, Wm, offset, part, lossd, stream);
    if (wave_loss) {                        // the three (kind 3: six) wave sums of crop_center(y), p (and crop_center(X))
        const float2 *xc = reinterpret_cast<const float2*>(xd), *yc = reinterpret_cast<const float2*>(yd), *pc = reinterpret_cast<const float2*>(od);
        float* w[3];
        for (int i = 0; i < wf.waves; ++i) w[i] = ws.allocf(wf.wave);
        float* wpart = ws.allocf(wf.part);
        float* table = ws.allocf(wf.table);
        if (wsdr_loss) launch_wave_term(plan, WaveTriple{xc, yc, nullptr, pc, T, offset, Wm, w[0], w[1], w[2], wpart}, table, &wave_host, signals, Wm, lossd + 1, stream);
        else launch_wave_term(plan, WavePair{pc, nullptr, yc, Wm, T, offset, w[0], w[1], wpart}, table, &wave_host, signals, Wm, lossd + 1, stream);
    }
    VR_HIP(hipMemcpyAsync(l4, lossd, (wsdr_loss ? 7 : wave_loss ? 4 : 1) * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    const float loss_h = wsdr_loss ? finish_wsdr_loss(l4) : wave_loss ? finish_wave_loss(l4) : l4[0];
    if (loss_out) *loss_out = loss_h;
}

// =====================================================================================================
// signal path
// =====================================================================================================
void Model::stft_api(const float* wave, bool on_dev, long long L, float* spec, bool spec_on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(L > 0, -2, "empty wave");
    const int T = 1 + (int)(L / hop);
    const size_t spec_f = (size_t)2 * output_bin * T * 2;
    ensure_io(((size_t)2 * L + spec_f) * sizeof(float) + 4096);
    io.reset();
    const float* wd = wave;
    if (!on_dev) {
        float* tmp = io.allocf((size_t)2 * L);
        VR_HIP(hipMemcpyAsync(tmp, wave, (size_t)2 * L * sizeof(float), hipMemcpyHostToDevice, stream));
        wd = tmp;
    }
    float* sd = spec_on_dev ? spec : io.allocf(spec_f);
    launch_stft(plan, wd, L, hop, T, reinterpret_cast<float2*>(sd), stream);
    if (!spec_on_dev) VR_HIP(hipMemcpyAsync(spec, sd, spec_f * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
}

void Model::istft_api(const float* spec, bool on_dev, int T, float* wave, bool wave_on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(T > 0, -2, "empty spectrogram");
    const size_t spec_f = (size_t)2 * output_bin * T * 2;
    const size_t out_f = (size_t)2 * hop * (T - 1);
    const size_t frames_f = (size_t)2 * T * n_fft;
    ensure_io((spec_f + out_f + frames_f) * sizeof(float) + 8192);
    io.reset();
    const float* sd = spec;
    if (!on_dev) {
        float* tmp = io.allocf(spec_f);
        VR_HIP(hipMemcpyAsync(tmp, spec, spec_f * sizeof(float), hipMemcpyHostToDevice, stream));
        sd = tmp;
    }
    float* frames = io.allocf(frames_f);
    float* wd = wave_on_dev ? wave : io.allocf(out_f + 4);
    launch_istft(plan, reinterpret_cast<const float2*>(sd), hop, T, frames, wd, stream);
    if (!wave_on_dev && out_f) VR_HIP(hipMemcpyAsync(wave, wd, out_f * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
}

// ---- WAV sample bytes in, PCM16 out (vr_*_pcm*): the format forms of the two tile kernels, csrc/pcm.h --------------------------------
bool Model::pcm_available() const { return istft_masked_available(plan, hop); }

// bytes: a DEVICE pointer to check for its samples' natural alignment, or null (host buffers are copied into the aligned staging arena)
void Model::check_pcm(const void* bytes, int channels, int fmt, const std::string& who) const {
    VR_CHECK(pcm_available(), -2, who + "the sample-format kernels are forms of the frame-tiled STFT / iSTFT, which this handle does not have "
                                        "(they need hop_length == n_fft / 2, n_fft >= 128, the tile inside the LDS budget, VR_NO_TILED_STFT "
                                        "unset: vr_pcm_available); convert on the host and use the float entry point");
    VR_CHECK(pcm_fmt_ok(fmt), -2, who + "unknown sample format " + std::to_string(fmt) + " (VR_PCM_S16 / S24 / S32 / F32)");
    VR_CHECK(channels == 1 || channels == 2, -2, who + "1 or 2 channels, not " + std::to_string(channels));
    if (bytes && fmt != VR_PCM_S24)
        VR_CHECK(reinterpret_cast<uintptr_t>(bytes) % (uintptr_t)pcm_sample_bytes(fmt) == 0, -2,
                 who + "the sample buffer is not aligned to its " + std::to_string(pcm_sample_bytes(fmt)) + "-byte samples (only VR_PCM_S24 may start at any byte)");
}

void Model::stft_pcm_api(const void* bytes, bool on_dev, long long L, int channels, int fmt, float* spec, bool spec_on_dev) {
    check_pcm(on_dev ? bytes : nullptr, channels, fmt, "");
    DeviceGuard dev_guard(device);
    VR_CHECK(L > 0, -2, "empty wave");
    VR_CHECK(L / hop < (1LL << 30), -2, "wave too long");
    const int T = 1 + (int)(L / hop);
    const size_t spec_f = (size_t)2 * output_bin * T * 2;
    const size_t in_b = (size_t)L * channels * pcm_sample_bytes(fmt);
    ensure_io(in_b + spec_f * sizeof(float) + 4096);
    io.reset();
    PcmIn in{static_cast<const uint8_t*>(bytes), channels, fmt};
    if (!on_dev) {
        void* tmp = io.alloc(in_b + 4);
        VR_HIP(hipMemcpyAsync(tmp, bytes, in_b, hipMemcpyHostToDevice, stream));
        in.bytes = static_cast<const uint8_t*>(tmp);
    }
    float* sd = spec_on_dev ? spec : io.allocf(spec_f);
    launch_stft_pcm(plan, in, L, T, reinterpret_cast<float2*>(sd), stream);
    if (!spec_on_dev) VR_HIP(hipMemcpyAsync(spec, sd, spec_f * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
}

void Model::istft_pcm16_api(const float* spec, bool on_dev, int T, int16_t* out, bool out_on_dev) {
    check_pcm(nullptr, 2, VR_PCM_S16, "");
    if (out_on_dev) VR_CHECK(reinterpret_cast<uintptr_t>(out) % 2 == 0, -2, "the int16 output is not 2-byte aligned");
    DeviceGuard dev_guard(device);
    VR_CHECK(T > 0, -2, "empty spectrogram");
    const size_t spec_f = (size_t)2 * output_bin * T * 2;
    const size_t out_n = (size_t)2 * hop * (T - 1);
    ensure_io(spec_f * sizeof(float) + out_n * 2 + 8192);
    io.reset();
    const float* sd = spec;
    if (!on_dev) {
        float* tmp = io.allocf(spec_f);
        VR_HIP(hipMemcpyAsync(tmp, spec, spec_f * sizeof(float), hipMemcpyHostToDevice, stream));
        sd = tmp;
    }
    int16_t* od = out_on_dev ? out : static_cast<int16_t*>(io.alloc(out_n * 2 + 16));
    launch_istft_masked_pcm16(plan, reinterpret_cast<const float2*>(sd), hop, T, false, nullptr, 0, nullptr, 0, 0, nullptr, 0, od, stream);
    if (!out_on_dev && out_n) VR_HIP(hipMemcpyAsync(out, od, out_n * 2, hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
}

// spec_utils.merge_artifacts (lib/spec_utils.py:60-93) reduced to its per-frame weight vector
// (the reference builds a [2, bins, T] weight that is constant over channel and bin).  numpy slice
// semantics are kept: negative starts wrap, a slice/linspace length mismatch is numpy's ValueError,
// an empty above-threshold set is the IndexError the reference raises at `idx[0]`.
void merge_artifacts_weight(const std::vector<float>& fmin, std::vector<float>& weight, float thres, int min_range,
                            int fade) {
    const int T = (int)fmin.size();
    VR_CHECK(min_range >= fade * 2, -2, "min_range must be >= fade_size * 2");
    weight.assign((size_t)T, 0.f);
    std::vector<int> idx;
    for (int t = 0; t < T; ++t) if (fmin[t] > thres) idx.push_back(t);
    VR_CHECK(!idx.empty(), -7, "index 0 is out of bounds for axis 0 with size 0");
    std::vector<int> starts{idx[0]}, ends;
    for (size_t i = 1; i < idx.size(); ++i)
        if (idx[i] - idx[i - 1] != 1) { ends.push_back(idx[i - 1]); starts.push_back(idx[i]); }
    ends.push_back(idx.back());
    auto norm = [T](int i) { if (i < 0) i += T; return i < 0 ? 0 : (i > T ? T : i); };
    auto assign_ramp = [&](int a, int b, bool up) {       // weight[a:b] = linspace(0,1,fade) or linspace(1,0,fade)
        const int lo = norm(a), hi = norm(b);
        const int n = hi > lo ? hi - lo : 0;
        VR_CHECK(n == fade, -2, "could not broadcast input array from shape (" + std::to_string(fade) + ",) into shape (" + std::to_string(n) + ",)");
        for (int i = 0; i < fade; ++i) {
            const double x = (double)i / (fade - 1);
            weight[lo + i] = (float)(up ? x : 1.0 - x);
        }
    };
    bool have_old = false;
    int old_e = 0;
    for (size_t k = 0; k < starts.size(); ++k) {
        int s0 = starts[k], e0 = ends[k];
        if (!(e0 - s0 > min_range)) continue;
        if (have_old && s0 - old_e < fade) s0 = old_e - fade * 2;
        if (s0 != 0) assign_ramp(s0, s0 + fade, true); else s0 -= fade;
        if (e0 != T) assign_ramp(e0 - fade, e0, false); else e0 += fade;
        const int lo = norm(s0 + fade), hi = norm(e0 - fade);
        for (int i = lo; i < hi; ++i) weight[i] = 1.f;
        old_e = e0;
        have_old = true;
    }
}

// dataset.make_padding (lib/dataset.py:198-205)
static void make_padding(int width, int cropsize, int offset, int& left, int& right, int& roi) {
    left = offset;
    roi = cropsize - offset * 2;
    if (roi == 0) roi = cropsize;
    right = roi - (width % roi) + left;
}

// The crops [0, patches) of a separate call in device batches of `bs`; run_crops(first, count) enqueues the network and the mask
// head for one contiguous part on the current streams.  A batch is split over the lanes unless profiling / serial_exec.
void Model::run_crop_chunks(int patches, int bs, const std::function<void(int, int)>& run_crops) {
    for (int i = 0; i < patches; i += bs) {
        const int nb = std::min(bs, patches - i);
        const int K = std::min((int)lanes.size() + 1, nb);
        if (K < 2 || profiling || serial) {
            run_crops(i, nb);
            continue;
        }
        // crops [i, i+nb) in K contiguous parts; part 0 on the handle's own streams, part j on lane j-1
        for (Lane& l : lanes) {
            if (l.ws.cap >= ws.cap) continue;            // every lane plans for the same (bs, cropsize)
            VR_HIP(hipDeviceSynchronize());
            if (l.ws.base) VR_HIP(hipFree(l.ws.base));
            l.ws.base = nullptr; l.ws.cap = 0;
            VR_HIP(hipMalloc(reinterpret_cast<void**>(&l.ws.base), ws.cap));
            l.ws.cap = ws.cap;
        }
        // The host enqueues part 0 completely before part 1 (~0.5 ms of launches: profiles/README.md), so the later lanes start late:
        // VR_LANE0_EXTRA = n gives part 0 n crops more than an even share.  Measured in round 6 (tools/gpu_r6_call7.sh, S30, two lanes):
        // 6 + 5 crops 8.63 - 8.78 ms, 7 + 4 8.69 - 8.73, 8 + 3 8.90; three lanes 10.4, one lane 9.24 -- the even split stays.
        static const int extra_env = getenv("VR_LANE0_EXTRA") ? atoi(getenv("VR_LANE0_EXTRA")) : -1;
        const int even = (nb + K - 1) / K;
        int head = extra_env >= 0 ? extra_env : 0;
        if (even + head > nb - (K - 1)) head = std::max(0, nb - (K - 1) - even);      // every part keeps at least one crop
        const int per0 = even + head;
        const int per = K > 1 ? (nb - per0 + K - 2) / (K - 1) : nb;
        for (int j = 1; j < K; ++j) {                    // `mag` is ready at this point of the main stream
            hipEvent_t es = lanes[j - 1].start;
            VR_HIP(hipEventRecord(es, stream));
            VR_HIP(hipStreamWaitEvent(lanes[j - 1].main, es, 0));
        }
        run_crops(i, std::min(per0, nb));
        for (int j = 1; j < K; ++j) {
            const int first = per0 + (j - 1) * per, count = std::min(per, nb - first);
            if (count <= 0) break;
            swap_lane(j - 1);
            try { run_crops(i + first, count); } catch (...) { swap_lane(j - 1); throw; }
            hipEvent_t done = lanes[j - 1].done;
            VR_HIP(hipEventRecord(done, stream));
            swap_lane(j - 1);
            VR_HIP(hipStreamWaitEvent(stream, done, 0));
        }
    }
}

void Model::mask_head(const Tensor& f3, int w_lo, int w_hi, HeadDst d) {
    d.w_lo = w_lo; d.w_hi = w_hi; d.pad_rows = output_bin - max_bin;
    if (is_complex) launch_head_complex(f3, out_w->dev, d, stream);
    else launch_head_sigmoid(f3, out_w->dev, d, stream);
}

void Model::crop_mask_head(const Tensor& f3, int cropsize, HeadDst d) { mask_head(f3, offset, cropsize - offset, d); }

void Model::run_dense_crops(float* dense, int count, int cropsize, const HeadDst& d) {
    ws.reset();
    Tensor x;
    x.p = dense; x.N = count; x.C = nin; x.H = max_bin; x.W = cropsize;
    x.sH = cropsize; x.sC = (long long)max_bin * cropsize; x.sN = x.C * x.sC;
    x.slope = 1.f;
    crop_mask_head(run_net_window(x, offset, cropsize - offset), cropsize, d);
}

// Separator.separate[_tta] / the inference.py:147-176 pipeline for n_songs inputs in ONE call: the executor of every offline entry
// point (vr_separate*, vr_separate*_many).  Each song keeps its own normaliser, padding and merge_artifacts runs; what the songs share
// is the device batches.  All crops of the call -- pass 0 of every song, then for tta pass 1 of every song -- form one list; a gather
// kernel writes the crops of a batch part as one dense tensor [n][nin][max_bin][cropsize] straight from the complex spectrograms
// (normalised, zero outside the song), and crop n's mask lands at column n * roi of one concatenated mask [2][bins][W].  Front end
// and back end are one launch each for all songs (song = a grid dimension, kernels.h SongSeg), so the launch count does not depend
// on n_songs.  solo: the call of a one-song entry point (api.cpp) -- its errors name no song, and its device batch holds at most the
// crops of its longer pass, which is what batchsize <= 0 means there.
// eval (vr_evaluate_wave*): a wave-level float call that also scores each song against its true instruments --
// the inst waves are staged like the mixtures, the back end is the evaluation form of the masked iSTFT plus one launch that adds its
// partials per window, and the sums go back to the host.  Without eval->stems no stem is allocated, stored or copied (y, v unused).
// pseudo (vr_pseudo*): the input of a song is a pair (X, Y) and the call returns P = Y + instruments stem of X - Y.  The
// front end stores Y and D = X - Y (wave level: the pair form of the tiled STFT; spectrogram level: one elementwise launch), the table's
// `spec` is D, so everything between the normaliser and the per-frame minima runs as for any song; the back end is the pseudo form
// of apply_mask, which stores P once, in the caller's layout.  No vocal stem and no wave is allocated, stored or copied (v unused).
// image (vr_separate_*_img): the call also returns the two spectrogram pictures of every song.  Nothing before the back
// end changes and no launch of it is replaced: two more launches (the range and the write form of mag_pad / apply_mask) read the song's
// spectrogram and the call's mask once more, and the pictures go out beside the stems.  Without image->stems no stem is formed at all.
void Model::separate_run(int n_songs, const float* const* in, bool in_on_dev, const int* T_in, const long long* L, int tta, int batchsize,
                         int cropsize, float* const* y, float* const* v, bool out_on_dev, const int* pcm_channels, const int* pcm_fmt,
                         bool solo, const EvalArgs* eval, const PseudoArgs* pseudo, const ImageArgs* image) {
    // VR_ENQ_TIMING=1 (diagnostics, wave-level calls): host time to ENQUEUE the whole call vs the time until the device has drained it
    static const bool enq_timing = getenv("VR_ENQ_TIMING") != nullptr;
    const auto enq_t0 = std::chrono::steady_clock::now();
    const bool post = (tta & 2) != 0;       // flags: bit 0 = --tta, bit 1 = --postprocess
    tta &= 1;
    const bool waves = L != nullptr;
    // vr_separate_pcm_many: in[s] are interleaved sample bytes (format and channel count per song), y[s] / v[s] int16 [samples][2]
    const bool pcm = pcm_fmt != nullptr;
    // ---- arguments and the host-side plan: nothing here touches the device
    VR_CHECK(n_songs > 0, -2, "n_songs must be positive");
    const bool stems = (!eval || eval->stems) && (!image || image->stems);
    if (image) VR_CHECK(!eval && !pseudo && image->y_img && image->v_img && (stems || waves), -2, "an image call takes songs and both picture tables");
    VR_CHECK(in && (!stems || (y && (v || pseudo))) && (waves || T_in), -2, "null table");
    if (pseudo) {
        VR_CHECK(!pcm && !eval && pseudo->inst, -2, "a pseudo-label call takes float pairs");
        VR_CHECK(pseudo->layout == 0 || pseudo->layout == 1, -2, "unknown layout");
        VR_CHECK(!waves || many_tiled_available(plan, hop), -2,
                 "the wave-level pseudo-label call needs hop_length == n_fft / 2 (the frame-tiled STFT kernel whose pair form it is exists only there)");
    }
    if (eval) {
        VR_CHECK(waves && !pcm && eval->inst && eval->sums, -2, "evaluation takes float waves and their true instruments");
        VR_CHECK(many_tiled_available(plan, hop), -2,
                 "evaluation needs hop_length == n_fft / 2 (the frame-tiled iSTFT kernel that forms the sums exists only there)");
        VR_CHECK(eval->window >= hop, -2, "window shorter than one hop");
    }
    VR_CHECK(!training, -2, "separate() runs in eval mode (inference.py:52); call vr_set_mode(h, 0) first");
    check_T(cropsize, offset, 1);
    VR_CHECK(cropsize - 2 * offset > 0, -6, "cropsize must exceed 2*offset");
    const int bins = output_bin, E = is_complex ? 2 : 1;
    struct Song { int T, pad_l, patches[2], crop0[2]; size_t spec_f, out_f; long long windows; };
    std::vector<Song> sg((size_t)n_songs);
    int roi = 0, max_T = 0;
    long long n_crops[2] = {0, 0}, sum_T = 0, sum_L = 0, max_windows = 0;
    auto song = [&](int s) { return solo ? std::string() : "song " + std::to_string(s) + ": "; };      // what an error starts with
    for (int s = 0; s < n_songs; ++s) {
        const std::string who = song(s);
        VR_CHECK(in[s] && (!stems || (y[s] && (pseudo || v[s]))) && (!eval || (eval->inst[s] && eval->sums[s])) && (!pseudo || pseudo->inst[s]), -2,
                 who + "null pointer");
        if (image) VR_CHECK(image->y_img[s] && image->v_img[s], -2, who + "null pointer");
        if (waves) VR_CHECK(L[s] >= hop, -2, who + "wave shorter than one hop");
        else VR_CHECK(T_in[s] > 0, -2, who + "empty spectrogram");
        if (waves) VR_CHECK(L[s] / hop < (1LL << 30), -2, who + "wave too long");
        if (pcm) {
            check_pcm(in_on_dev ? in[s] : nullptr, pcm_channels[s], pcm_fmt[s], who);
            if (out_on_dev && stems) VR_CHECK(reinterpret_cast<uintptr_t>(y[s]) % 2 == 0 && reinterpret_cast<uintptr_t>(v[s]) % 2 == 0, -2, who + "the int16 outputs are not 2-byte aligned");
        }
        Song& g = sg[s];
        g.T = waves ? 1 + (int)(L[s] / hop) : T_in[s];
        int pad_r;
        make_padding(g.T, cropsize, offset, g.pad_l, pad_r, roi);
        g.patches[0] = (g.T + g.pad_l + pad_r - 2 * offset) / roi;
        g.patches[1] = tta ? (g.T + g.pad_l + pad_r + roi - 2 * offset) / roi : 0;
        g.spec_f = (size_t)2 * bins * g.T * 2;
        g.out_f = (size_t)2 * hop * (g.T - 1);
        g.windows = eval ? evaluate_plan(hop, L[s], eval->window).windows : 0;
        max_windows = std::max(max_windows, g.windows);
        max_T = std::max(max_T, g.T);
        sum_T += g.T;
        if (waves) sum_L += L[s];
    }
    for (int ps = 0; ps < 2; ++ps)
        for (int s = 0; s < n_songs; ++s) { sg[s].crop0[ps] = (int)(n_crops[0] + n_crops[1]); n_crops[ps] += sg[s].patches[ps]; }
    const long long total_crops = n_crops[0] + n_crops[1];
    VR_CHECK(total_crops * roi < (1LL << 31) && sum_T < (1LL << 31), -2, "too many frames for one call: split the songs over several calls");
    const int crops_n = (int)total_crops, W = crops_n * roi;
    const int most = solo ? std::max(sg[0].patches[0], sg[0].patches[1]) : crops_n;
    const int bs = (batchsize <= 0) ? most : std::min(batchsize, most);
    const bool tiled = many_tiled_available(plan, hop);

    DeviceGuard dev_guard(device);
    // ---- the staging arena: carved twice, first dry for its size
    std::vector<SongSeg> tab((size_t)n_songs);
    std::vector<float*> stage_in((size_t)n_songs), stage_y((size_t)n_songs), stage_v((size_t)n_songs);
    SongSeg* tab_d = nullptr; int2* crops_d = nullptr;
    std::vector<PcmIn> pin(pcm ? (size_t)n_songs : 0);
    PcmIn* pin_d = nullptr;
    std::vector<WaveEval> evt(eval ? (size_t)n_songs : 0);
    std::vector<float*> stage_inst(eval ? (size_t)n_songs : 0);
    WaveEval* evt_d = nullptr;
    std::vector<PseudoSeg> pst(pseudo ? (size_t)n_songs : 0);
    std::vector<float*> stage_pinst(pseudo ? (size_t)n_songs : 0);
    PseudoSeg* pst_d = nullptr;
    std::vector<ImgSeg> imt(image ? (size_t)n_songs : 0);
    ImgSeg* imt_d = nullptr;
    float* img_range = nullptr;
    double pcm_bytes = 0.0;
    auto in_bytes = [&](int s) {
        return pcm ? (size_t)L[s] * pcm_channels[s] * pcm_sample_bytes(pcm_fmt[s]) : (waves ? (size_t)2 * L[s] : sg[s].spec_f) * sizeof(float);
    };
    unsigned long long* part = nullptr;
    float *aff = nullptr, *mask = nullptr, *gather = nullptr, *fmin_d = nullptr, *wgt_d = nullptr, *frames = nullptr;
    const size_t crop_f = (size_t)nin * max_bin * cropsize;
    auto carve = [&](Arena& A) {
        tab_d = static_cast<SongSeg*>(A.alloc(sizeof(SongSeg) * n_songs));
        crops_d = static_cast<int2*>(A.alloc(sizeof(int2) * crops_n));
        if (pcm) pin_d = static_cast<PcmIn*>(A.alloc(sizeof(PcmIn) * n_songs));
        if (eval) evt_d = static_cast<WaveEval*>(A.alloc(sizeof(WaveEval) * n_songs));
        if (pseudo) pst_d = static_cast<PseudoSeg*>(A.alloc(sizeof(PseudoSeg) * n_songs));
        if (image) {                                  // one job per song beside the table: two pictures, their partials and ranges
            imt_d = static_cast<ImgSeg*>(A.alloc(sizeof(ImgSeg) * n_songs));
            img_range = A.allocf((size_t)n_songs * 4);
            for (int s = 0; s < n_songs; ++s) {
                const size_t bytes = (size_t)3 * bins * sg[s].T;
                ImgSeg& e = imt[s];
                e = ImgSeg{};
                e.T = sg[s].T;
                e.img[0] = out_on_dev ? image->y_img[s] : static_cast<uint8_t*>(A.alloc(bytes));
                e.img[1] = out_on_dev ? image->v_img[s] : static_cast<uint8_t*>(A.alloc(bytes));
                e.part = static_cast<float4*>(A.alloc(sizeof(float4) * kImgParts));
                e.range = img_range + 4 * s;
            }
        }
        part = static_cast<unsigned long long*>(A.alloc((size_t)n_songs * 2 * bins * 16));
        aff = A.allocf((size_t)n_songs * 4);
        mask = A.allocf((size_t)E * 2 * bins * W);
        gather = A.allocf((size_t)bs * crop_f + 4096);
        if (post) { fmin_d = A.allocf((size_t)sum_T); wgt_d = A.allocf((size_t)sum_T); }
        if (waves && !tiled) frames = A.allocf((size_t)2 * max_T * n_fft);
        for (int s = 0; s < n_songs; ++s) {
            const Song& g = sg[s];
            SongSeg& t = tab[s];
            t = SongSeg{};
            t.T = g.T;
            t.mcol_a = g.crop0[0] * roi;
            t.mcol_b = tta ? g.crop0[1] * roi + roi / 2 : 0;
            stage_in[s] = in_on_dev ? nullptr : A.allocf(in_bytes(s) / 4 + (pcm ? 1 : 0));
            const float* src = in_on_dev ? in[s] : stage_in[s];
            if (pseudo) {                             // the pair beside the table entry: `spec` is D, P goes out once, no other stem exists
                stage_pinst[s] = in_on_dev ? nullptr : A.allocf(in_bytes(s) / 4);
                const float* isrc = in_on_dev ? pseudo->inst[s] : stage_pinst[s];
                PseudoSeg& q = pst[s];
                q = PseudoSeg{};
                t.spec = reinterpret_cast<float2*>(A.allocf(g.spec_f));
                if (waves) {
                    t.wave = src; t.L = L[s];
                    q.inst_wave = isrc;
                    q.inst = reinterpret_cast<float2*>(A.allocf(g.spec_f));
                } else {
                    q.mix = reinterpret_cast<const float2*>(src);
                    q.inst = reinterpret_cast<float2*>(const_cast<float*>(isrc));
                }
                stage_y[s] = out_on_dev ? y[s] : A.allocf(g.spec_f);
                q.out = reinterpret_cast<float2*>(stage_y[s]);
            } else if (waves) {
                t.wave = src; t.L = L[s];
                if (pcm) {                            // the STFT reads the bytes through the PcmIn table; the stems are int16
                    t.wave = nullptr;
                    pin[s] = PcmIn{reinterpret_cast<const uint8_t*>(src), pcm_channels[s], pcm_fmt[s]};
                }
                t.spec = reinterpret_cast<float2*>(A.allocf(g.spec_f));
                if (stems) {
                    stage_y[s] = out_on_dev ? y[s] : A.allocf((pcm ? g.out_f / 2 : g.out_f) + 4);
                    stage_v[s] = out_on_dev ? v[s] : A.allocf((pcm ? g.out_f / 2 : g.out_f) + 4);
                }
                t.y_wave = stage_y[s]; t.v_wave = stage_v[s];
                if (eval) {                           // the true instruments beside the mixture; the partials and the sums of this song
                    stage_inst[s] = in_on_dev ? nullptr : A.allocf((size_t)2 * L[s]);
                    WaveEval& e = evt[s];
                    e.inst = in_on_dev ? eval->inst[s] : stage_inst[s];
                    e.part = static_cast<double*>(A.alloc(eval_part_doubles(g.T) * sizeof(double)));
                    e.sums = static_cast<double*>(A.alloc((size_t)g.windows * 4 * sizeof(double)));
                    e.window = eval->window;
                    e.store = stems ? 1 : 0;
                }
                if (!tiled) {                         // general hop: masked spectrograms, then the per-frame inverse per song
                    t.y = reinterpret_cast<float2*>(A.allocf(g.spec_f));
                    t.v = reinterpret_cast<float2*>(A.allocf(g.spec_f));
                }
            } else {
                t.spec = reinterpret_cast<float2*>(const_cast<float*>(src));
                stage_y[s] = out_on_dev ? y[s] : A.allocf(g.spec_f);
                stage_v[s] = out_on_dev ? v[s] : A.allocf(g.spec_f);
                t.y = reinterpret_cast<float2*>(stage_y[s]); t.v = reinterpret_cast<float2*>(stage_v[s]);
            }
        }
    };
    Arena dry;
    dry.dry = true;
    carve(dry);
    ensure_io(dry.peak + 65536);
    io.reset();
    carve(io);
    std::vector<int2> crops((size_t)crops_n);
    int frame0 = 0;
    for (int s = 0; s < n_songs; ++s) {
        tab[s].frame0 = frame0;
        if (post) tab[s].fmin = fmin_d + frame0;
        frame0 += sg[s].T;
        for (int ps = 0; ps < (tta ? 2 : 1); ++ps)
            for (int i = 0; i < sg[s].patches[ps]; ++i)
                crops[(size_t)sg[s].crop0[ps] + i] = make_int2(s, i * roi - sg[s].pad_l - (ps ? roi / 2 : 0));
    }
    VR_HIP(hipMemcpyAsync(tab_d, tab.data(), sizeof(SongSeg) * n_songs, hipMemcpyHostToDevice, stream));
    VR_HIP(hipMemcpyAsync(crops_d, crops.data(), sizeof(int2) * crops_n, hipMemcpyHostToDevice, stream));
    if (pcm) {
        VR_HIP(hipMemcpyAsync(pin_d, pin.data(), sizeof(PcmIn) * n_songs, hipMemcpyHostToDevice, stream));
        for (int s = 0; s < n_songs; ++s) pcm_bytes += (double)in_bytes(s);
    }
    if (!in_on_dev)
        for (int s = 0; s < n_songs; ++s)
            VR_HIP(hipMemcpyAsync(stage_in[s], in[s], in_bytes(s), hipMemcpyHostToDevice, stream));
    if (eval) {
        VR_HIP(hipMemcpyAsync(evt_d, evt.data(), sizeof(WaveEval) * n_songs, hipMemcpyHostToDevice, stream));
        if (!in_on_dev)
            for (int s = 0; s < n_songs; ++s)
                VR_HIP(hipMemcpyAsync(stage_inst[s], eval->inst[s], in_bytes(s), hipMemcpyHostToDevice, stream));
    }
    if (pseudo) {
        VR_HIP(hipMemcpyAsync(pst_d, pst.data(), sizeof(PseudoSeg) * n_songs, hipMemcpyHostToDevice, stream));
        if (!in_on_dev)
            for (int s = 0; s < n_songs; ++s)
                VR_HIP(hipMemcpyAsync(stage_pinst[s], pseudo->inst[s], in_bytes(s), hipMemcpyHostToDevice, stream));
    }
    if (image) VR_HIP(hipMemcpyAsync(imt_d, imt.data(), sizeof(ImgSeg) * n_songs, hipMemcpyHostToDevice, stream));
    // ---- front end
    if (pseudo) {                           // Y and D = X - Y; X itself is never written (waves: tiled, checked above)
        if (waves) launch_stft_pseudo_many(plan, tab_d, pst_d, n_songs, max_T, (double)sum_L, (double)sum_T, stream);
        else launch_pseudo_diff_many(tab_d, pst_d, n_songs, bins, (double)sum_T, stream);
    } else if (waves) {
        if (pcm) launch_stft_many(plan, tab_d, n_songs, max_T, (double)sum_L, (double)sum_T, stream, pin_d, pcm_bytes);   // (check_pcm: tiled)
        else if (tiled) launch_stft_many(plan, tab_d, n_songs, max_T, (double)sum_L, (double)sum_T, stream);
        else for (int s = 0; s < n_songs; ++s) launch_stft(plan, tab[s].wave, L[s], hop, sg[s].T, tab[s].spec, stream);
    }
    launch_song_stats(tab_d, n_songs, bins, (double)sum_T, part, stream);
    launch_song_coef(part, n_songs, 2 * bins, tta ? 1 : 0, is_complex, aff, stream);
    // ---- the network over the crop list
    fold_eval_affines();                    // before planning, as in forward_api
    plan_and_reserve(bs, cropsize, 0);
    auto run_crops = [&](int first, int count) {
        float* dense = gather + (size_t)(first % bs) * crop_f;          // (batches start at multiples of bs: the part's slot in its batch)
        launch_crop_gather(tab_d, crops_d + first, count, is_complex, bins, max_bin, cropsize, aff, dense, stream);
        HeadDst d{};
        d.p = mask + (size_t)E * first * roi; d.dN = roi; d.dC = (long long)bins * W; d.dH = W;
        run_dense_crops(dense, count, cropsize, d);
    };
    run_crop_chunks(crops_n, bs, run_crops);
    // ---- back end
    const float* wgt = nullptr;
    std::vector<float> fmin_h, wgt_h;
    if (post) {
        launch_frame_min_many(tab_d, n_songs, max_T, bins, mask, W, tta, is_complex, stream);
        fmin_h.resize((size_t)sum_T);
        wgt_h.resize((size_t)sum_T);
        VR_HIP(hipMemcpyAsync(fmin_h.data(), fmin_d, (size_t)sum_T * sizeof(float), hipMemcpyDeviceToHost, stream));
        VR_HIP(hipStreamSynchronize(stream));
        std::vector<float> f1, w1;
        for (int s = 0; s < n_songs; ++s) {
            f1.assign(fmin_h.begin() + tab[s].frame0, fmin_h.begin() + tab[s].frame0 + sg[s].T);
            try {
                merge_artifacts_weight(f1, w1, 0.05f, 64, 32);
            } catch (const Error& e) {
                throw Error(e.code, song(s) + e.what());
            }
            std::copy(w1.begin(), w1.end(), wgt_h.begin() + tab[s].frame0);
        }
        VR_HIP(hipMemcpyAsync(wgt_d, wgt_h.data(), (size_t)sum_T * sizeof(float), hipMemcpyHostToDevice, stream));
        wgt = wgt_d;
    }
    if (pseudo) {
        launch_apply_mask_pseudo_many(tab_d, pst_d, n_songs, max_T, bins, mask, W, tta, is_complex, wgt, pseudo->layout == 1, (double)sum_T, stream);
    } else if (eval) {                      // (tiled, checked above)
        for (int which = 0; which < 2; ++which)
            launch_istft_eval_many(plan, tab_d, evt_d, n_songs, max_T, (double)sum_T, mask, W, tta ? mask : nullptr, W, 0, is_complex, wgt, which,
                                   stems, stream);
        launch_eval_sums(plan, tab_d, evt_d, n_songs, max_windows, (double)sum_T, stream);
        for (int s = 0; s < n_songs; ++s)
            if (sg[s].windows)
                VR_HIP(hipMemcpyAsync(eval->sums[s], evt[s].sums, (size_t)sg[s].windows * 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
    } else if (waves && tiled) {
        for (int which = 0; which < 2 && stems; ++which)
            launch_istft_masked_many(plan, tab_d, n_songs, max_T, (double)sum_T, mask, W, tta, is_complex, wgt, which, stream, pcm);
    } else if (stems) {
        launch_apply_mask_many(tab_d, n_songs, max_T, bins, mask, W, tta, is_complex, wgt, stream);
        if (waves)
            for (int s = 0; s < n_songs; ++s) {
                launch_istft(plan, tab[s].y, hop, sg[s].T, frames, tab[s].y_wave, stream);
                launch_istft(plan, tab[s].v, hop, sg[s].T, frames, tab[s].v_wave, stream);
            }
    }
    if (image) {                            // the pictures of the very stems, from the resident spectrogram and mask: no stem is stored for them
        launch_stem_image_many(tab_d, imt_d, n_songs, max_T, bins, mask, W, tta, is_complex, wgt, (double)sum_T, stream);
        if (!out_on_dev)
            for (int s = 0; s < n_songs; ++s) {
                VR_HIP(hipMemcpyAsync(image->y_img[s], imt[s].img[0], (size_t)3 * bins * sg[s].T, hipMemcpyDeviceToHost, stream));
                VR_HIP(hipMemcpyAsync(image->v_img[s], imt[s].img[1], (size_t)3 * bins * sg[s].T, hipMemcpyDeviceToHost, stream));
            }
        if (image->ranges) VR_HIP(hipMemcpyAsync(image->ranges, img_range, (size_t)n_songs * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    if (!out_on_dev && stems)
        for (int s = 0; s < n_songs; ++s) {
            const size_t nf = (waves && !pseudo) ? sg[s].out_f : sg[s].spec_f;
            if (!nf) continue;
            VR_HIP(hipMemcpyAsync(y[s], stage_y[s], nf * (pcm ? 2 : sizeof(float)), hipMemcpyDeviceToHost, stream));
            if (pseudo) continue;
            VR_HIP(hipMemcpyAsync(v[s], stage_v[s], nf * (pcm ? 2 : sizeof(float)), hipMemcpyDeviceToHost, stream));
        }
    const auto enq_t1 = std::chrono::steady_clock::now();     // everything is enqueued at this point
    VR_HIP(hipStreamSynchronize(stream));
    if (enq_timing && waves)
        fprintf(stderr, "[vr-enq] enqueue %.3f ms, total %.3f ms\n", std::chrono::duration<double, std::milli>(enq_t1 - enq_t0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - enq_t0).count());
}

EvalPlan evaluate_plan(int hop, long long L, long long window) {
    VR_CHECK(hop > 0, -2, "hop must be positive");
    VR_CHECK(L >= hop, -2, "wave shorter than one hop");
    VR_CHECK(window >= hop, -2, "window shorter than one hop");
    EvalPlan p{};
    p.samples = (long long)hop * (L / hop);
    p.windows = p.samples / window + (p.samples % window ? 1 : 0);
    return p;
}

// =====================================================================================================
// Streaming separation (vr_stream_*): audio is pushed in blocks, stems come back as soon as they are final.
// The offline call's crops sit at multiples of roi whatever the song's length, and the only whole-song quantity is the normaliser:
// given it, a stream runs the same crops on the same numbers.  Per stream the device keeps an input tail, a ring of spectrogram
// frames, a mask ring per pass, one hop of overlap-add carry per stem and channel, and the normaliser (StreamState); the staging
// arena holds one push.  A push is cut into steps of at most `chunk_frames` new frames, so the rings have a fixed size; a step is
// one STFT of the new frames, one statistics launch (running normaliser / MEASURE), the ready crops through run_crop_chunks, and one
// masked iSTFT per stem over the frames that became final.  One executor runs them, stream_run: vr_stream_push gives it one stream,
// vr_stream_push_many a round of streams.  A --postprocess stream gives its frames out kStreamPostDelay behind
// their masks (`out_done` behind `done`): in front of the iSTFT a step takes the minima of the mask columns that became final and walks
// them into merge_artifacts weights (stream_post.h), both in rings beside the others.
// =====================================================================================================
StreamSchedule stream_schedule(int n_fft, int hop, int cropsize, int offset, int tta, long long samples_in, int flushed, int postprocess) {
    VR_CHECK(n_fft >= 2 && hop > 0 && hop * 2 == n_fft, -2, "streaming needs hop_length == n_fft / 2 (the frame-tiled STFT / iSTFT kernels exist only there)");
    VR_CHECK(offset >= 0 && cropsize - 2 * offset > 0, -2, "cropsize must exceed 2*offset");
    VR_CHECK(samples_in >= 0, -2, "negative sample count");
    VR_CHECK(!flushed || samples_in >= hop, -2, "wave shorter than one hop");
    const long long roi = cropsize - 2 * offset, half = roi / 2;
    StreamSchedule p{};
    p.frames = samples_in / hop + (flushed ? 1 : 0);
    if (flushed) {
        p.crops[0] = p.frames / roi + 1;
        p.crops[1] = tta ? p.frames / roi + 2 : 0;
        p.done = p.frames;
    } else {
        p.crops[0] = p.frames >= offset ? (p.frames - offset) / roi : 0;
        p.crops[1] = (tta && p.frames + half >= offset) ? (p.frames - offset + half) / roi : 0;
        p.done = tta ? std::max(0LL, std::min(p.crops[0] * roi, p.crops[1] * roi - half)) : p.crops[0] * roi;
    }
    p.out_done = p.done;
    if (postprocess && !flushed) p.out_done = p.done - kStreamPostDelay >= 2 ? p.done - kStreamPostDelay : 0;
    p.samples_out = (long long)hop * std::max(0LL, p.out_done - 1);
    return p;
}

static unsigned host_ord32(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static float host_unord32(unsigned o) {
    const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

StreamState* Model::stream_open(int cropsize, int batchsize, int flags, double coef_re, double coef_im) {
    // ---- arguments: nothing here touches the device
    VR_CHECK(!(flags & ~15), -2, "unknown vr_stream_open flag");
    VR_CHECK(!((flags & 8) && (flags & 2)), -2, "VR_STREAM_PCM16_OUT on a VR_STREAM_MEASURE stream: it returns no samples");
    VR_CHECK(!((flags & 4) && (flags & 2)), -2, "VR_STREAM_POSTPROCESS on a VR_STREAM_MEASURE stream: it returns no samples to post-process");
    VR_CHECK(!training, -2, "a stream runs in eval mode (inference.py:52); call vr_set_mode(h, 0) first");
    VR_CHECK(hop * 2 == n_fft && stream_tiled_available(plan, hop), -2,
             "streaming needs hop_length == n_fft / 2 (the frame-tiled STFT / iSTFT kernels exist only there)");
    check_T(cropsize, offset, 1);
    VR_CHECK(cropsize - 2 * offset > 0, -6, "cropsize must exceed 2*offset");
    const bool tta = flags & 1, measure = (flags & 2) != 0;
    const bool running = !measure && coef_re == 0.0 && coef_im == 0.0;
    VR_CHECK(!(running && tta), -2, "a tta stream needs the normaliser (coef): the running normaliser exists for plain streams only");
    VR_CHECK(!(running && (flags & 4)), -2, "a postprocess stream needs the normaliser (coef): with the running normaliser a step ends with "
                                           "every crop window, and the look-ahead of merge_artifacts is not worked out for it");
    VR_CHECK(measure || (std::isfinite(coef_re) && std::isfinite(coef_im)), -2, "coef must be finite");
    std::unique_ptr<StreamState> S(new StreamState);
    S->cropsize = cropsize; S->tta = tta; S->measure = measure; S->running = running;
    S->pcm16 = (flags & 8) != 0;                // y / v are int16 [capacity][2]: the last kernel's store encodes
    S->post = (flags & 4) != 0;                 // merge_artifacts with kStreamPostDelay frames of look-ahead
    S->bs = batchsize > 0 ? batchsize : 8;               // (a stream never sees "all crops": <= 0 means 8)
    const int roi = cropsize - 2 * offset, bins = output_bin, E = is_complex ? 2 : 1;
    S->roi = roi;
    S->chunk_frames = S->bs * roi;
    // frames still needed before a step reach back less than cropsize + roi / 2, a step adds at most chunk_frames (+ 1 at flush)
    // (post: frames leave kStreamPostDelay behind their masks, so both rings keep that many more)
    S->R = cropsize + roi / 2 + S->chunk_frames + 4 + (S->post ? kStreamPostDelay : 0);
    // mask columns not yet final before a step: at most roi / 2; a step adds at most bs + 1 crops per pass, the flush offset / roi + 3
    S->RM = roi * (std::max(S->bs + 1, offset / roi + 3) + 2 + (S->post ? (kStreamPostDelay + roi - 1) / roi : 0));
    // minima and weights: from the oldest frame not yet out to the newest final mask, which is what the frame ring spans
    S->RW = S->post ? S->R : 0;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t a = (off + 255) & ~size_t(255); off = a + bytes; return a; };
    const size_t tail_b = (size_t)2 * 2 * hop * 4, ring_b = (size_t)2 * bins * S->R * 8, mask_b = (size_t)E * 2 * bins * S->RM * 4;
    const size_t carry_b = (size_t)2 * 2 * hop * 4, stats_b = 16 + (size_t)2 * bins * 16;
    const size_t o_tail0 = take(tail_b), o_tail1 = take(tail_b), o_ring = take(ring_b);
    const size_t o_stats = take(stats_b), o_aff = take(64);
    size_t o_mask[2] = {0, 0}, o_carry[2] = {0, 0};
    if (!measure) {
        o_mask[0] = take(mask_b);
        if (tta) o_mask[1] = take(mask_b);
        o_carry[0] = take(carry_b); o_carry[1] = take(carry_b);
    }
    size_t o_fmin = 0, o_wgt = 0, o_post = 0;
    if (S->post) { o_fmin = take((size_t)S->RW * 4); o_wgt = take((size_t)S->RW * 4); o_post = take(sizeof(StreamPostState)); }
    S->state_bytes = off;

    DeviceGuard dev_guard(device);
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&S->slab), off));
    try {
        char* b = S->slab;
        S->tail[0] = reinterpret_cast<float*>(b + o_tail0); S->tail[1] = reinterpret_cast<float*>(b + o_tail1);
        S->ring = reinterpret_cast<float2*>(b + o_ring);
        S->stats = reinterpret_cast<unsigned*>(b + o_stats); S->aff = reinterpret_cast<float*>(b + o_aff);
        if (!measure) {
            S->mask[0] = reinterpret_cast<float*>(b + o_mask[0]);
            S->mask[1] = tta ? reinterpret_cast<float*>(b + o_mask[1]) : nullptr;
            S->carry[0] = reinterpret_cast<float*>(b + o_carry[0]); S->carry[1] = reinterpret_cast<float*>(b + o_carry[1]);
        }
        if (S->post) {                          // (the zeroed slab is the walk's state before frame 0)
            S->fmin_ring = reinterpret_cast<float*>(b + o_fmin); S->wgt_ring = reinterpret_cast<float*>(b + o_wgt);
            S->post_state = reinterpret_cast<StreamPostState*>(b + o_post);
        }
        VR_HIP(hipMemsetAsync(S->slab, 0, off, stream));
        // the statistics rows as an empty reduction leaves them (the zero padding is part of the reduced array); a given normaliser
        // enters as row 0, so that 1 / c comes from the same coef_affine arithmetic as offline
        std::vector<unsigned long long> st((size_t)2 + 2 * 2 * bins);
        const unsigned long long zero_key = ((unsigned long long)host_ord32(0.f) << 32) | host_ord32(0.f);
        st[0] = st[1] = 0;
        for (int r = 0; r < 2 * bins; ++r) { st[2 + 2 * r] = 0; st[2 + 2 * r + 1] = zero_key; }
        if (!measure && !running) {
            const float re = (float)coef_re, im = (float)coef_im;
            float mag = (float)std::hypot(coef_re, coef_im);
            if (coef_im == 0.0) mag = std::fabs(re);
            unsigned mb;
            memcpy(&mb, &mag, 4);
            st[2] = mb;
            const unsigned long long key = ((unsigned long long)host_ord32(re) << 32) | host_ord32(im);
            st[3] = key > zero_key ? key : zero_key;
            VR_CHECK(mag > 0.f, -2, "coef must not be zero");
        }
        VR_HIP(hipMemcpyAsync(S->stats, st.data(), st.size() * 8, hipMemcpyHostToDevice, stream));
        if (!measure && !running) {
            if (is_complex) launch_coef_complex(S->stats, 2 * bins, tta ? 1 : 0, reinterpret_cast<float2*>(S->aff), stream);
            else launch_coef_affine(S->stats, 2 * bins, tta ? 1 : 0, S->aff, stream);
        }
        VR_HIP(hipStreamSynchronize(stream));
    } catch (...) {
        hipFree(S->slab);
        throw;
    }
    return S.release();
}

void Model::stream_close(StreamState* S) {
    if (!S) return;
    DeviceGuard dev_guard(device);
    hipStreamSynchronize(stream);
    if (S->slab) hipFree(S->slab);
    delete S;
}

Model::StreamStepPlan Model::stream_step_plan(StreamState& S, const StreamStepIO& o, bool final) {
    const int roi = S.roi, cropsize = S.cropsize;
    const long long prev_frames = S.frames;
    S.samples += o.blk_n;
    StreamStepPlan sp{};
    const StreamSchedule p = stream_schedule(n_fft, hop, cropsize, offset, S.tta, S.samples, final, S.post);
    sp.p = p;
    VR_CHECK(p.frames < (1LL << 31) - 2 * cropsize, -2, "stream too long");
    // what the rings must still hold: the oldest frame a coming crop or the iSTFT reads, the oldest mask column not yet final
    long long oldest = std::min(S.out_done, S.crops[0] * roi - offset);
    if (S.tta) oldest = std::min(oldest, S.crops[1] * roi - offset - roi / 2);
    if (S.measure) oldest = prev_frames;        // (only the statistics pass reads the new frames)
    VR_CHECK(p.frames - std::max(0LL, oldest) <= S.R, -4, "stream frame ring overflow (planning bug)");
    if (!S.measure) {
        VR_CHECK(p.crops[0] * roi - S.out_done / roi * roi <= S.RM, -4, "stream mask ring overflow (planning bug)");
        if (S.tta) VR_CHECK(p.crops[1] * roi - (S.out_done + roi / 2) / roi * roi <= S.RM, -4, "stream mask ring overflow (planning bug)");
        if (S.post) VR_CHECK(p.done - S.out_done <= S.RW, -4, "stream weight ring overflow (planning bug)");
        VR_CHECK((p.crops[0] - S.crops[0]) + (p.crops[1] - S.crops[1]) <= 2 * (S.RM / roi), -4, "stream crop list overflow (planning bug)");
    }
    StreamSeg& g = sp.seg;
    g.tail = S.tail[S.tail_cur]; g.tail_out = S.tail[S.tail_cur ^ 1];
    g.blk = o.blk; g.blk_pitch = o.blk_pitch;
    g.tail_base = S.tail_base; g.blk_base = S.samples - o.blk_n;
    g.tail_out_base = std::max(0LL, (S.samples / hop - 1) * hop);
    g.L = S.samples; g.tail_pitch = 2 * hop;
    g.ring = S.ring; g.R = S.R; g.t_new = (int)prev_frames; g.T = (int)p.frames;
    g.mask_a = S.mask[0]; g.mask_b = S.tta ? S.mask[1] : nullptr; g.RM = S.RM; g.shift = roi / 2;
    g.aff = S.aff;
    sp.emit = !S.measure && p.out_done > S.out_done;
    g.carried = S.out_done > 0;
    g.t_out = S.out_done > 0 ? (int)S.out_done - 1 : 0; g.t_done = (int)p.out_done;
    g.carry_in = S.carry[S.carry_cur]; g.carry_out = S.carry[S.carry_cur ^ 1];
    g.y_wave = o.y ? o.y + o.out_off : nullptr; g.v_wave = o.v ? o.v + o.out_off : nullptr; g.out_pitch = o.out_pitch;
    sp.new_frames = (int)(p.frames - prev_frames);
    sp.segments = sp.emit ? g.t_done - 1 - g.t_out : 0;
    if (S.post) {
        g.fmin_ring = S.fmin_ring; g.wgt_ring = S.wgt_ring; g.post = S.post_state; g.RW = S.RW;
        g.fm_lo = (int)S.done; g.fm_hi = (int)p.done; g.post_flush = final;
        sp.post_frames = (int)(p.done - S.done);
        sp.post_walk = sp.post_frames > 0 || final;
    }
    return sp;
}

// the crops that became ready in this step: pass 0, then pass 1
void Model::stream_step_crops(const StreamState& S, const StreamStepPlan& sp, int entry, std::vector<StreamCrop>& list) const {
    if (S.measure) return;
    for (int ps = 0; ps < (S.tta ? 2 : 1); ++ps)
        for (long long i = S.crops[ps]; i < sp.p.crops[ps]; ++i) list.push_back(StreamCrop{entry, ps, i});
}

void Model::stream_step_commit(StreamState& S, StreamStepIO& o, const StreamStepPlan& sp) {
    if (sp.emit) {
        S.carry_cur ^= 1;
        o.out_off += (long long)hop * sp.segments;
        S.out_done = sp.p.out_done;
    }
    if (!S.measure) S.done = sp.p.done;
    S.tail_cur ^= 1;
    S.tail_base = sp.seg.tail_out_base;
    S.frames = sp.p.frames; S.crops[0] = sp.p.crops[0]; S.crops[1] = sp.p.crops[1];
}

// The checks of one stream's share of a push call that vr_stream_push and vr_stream_push_many have in common, `who` in front of
// every message; nothing here touches the device or the stream.
long long Model::stream_check(const StreamState& S, const std::string& who, const float* wave, long long n, bool flush, const float* y,
                              const float* v, bool out_on_dev, long long capacity) const {
    VR_CHECK(!S.broken, -2, who + "this stream failed in an earlier call: close it");
    VR_CHECK(!S.flushed, -2, who + (flush ? "the stream is already flushed" : "push after flush"));
    VR_CHECK(n >= 0 && (n == 0 || wave), -2, who + "null or negative input");
    long long need = 0;
    try {
        const StreamSchedule before = stream_schedule(n_fft, hop, S.cropsize, offset, S.tta, S.samples, 0, S.post);
        const StreamSchedule after = stream_schedule(n_fft, hop, S.cropsize, offset, S.tta, S.samples + n, flush, S.post);
        need = S.measure ? 0 : after.samples_out - before.samples_out;
    } catch (const Error& e) {
        throw Error(e.code, who + e.what());
    }
    if (need > 0)
        VR_CHECK(y && v && capacity >= need, -2, who + "output capacity " + std::to_string(capacity) + " is too small: this call returns " +
                                                     std::to_string(need) + " samples per channel");
    if (S.pcm16 && need > 0 && out_on_dev)
        VR_CHECK(reinterpret_cast<uintptr_t>(y) % 2 == 0 && reinterpret_cast<uintptr_t>(v) % 2 == 0, -2, who + "the int16 outputs are not 2-byte aligned");
    return need;
}

// The steps of the streams of one push call, taken together in rounds.  Round r holds step r of every part that still has one -- at
// most chunk_frames new frames, the flush step last -- so a stream's steps, and with them its crops and its numbers, are the same
// whichever streams share the call; what the parts share is the launches: one StreamSeg table and one crop list per round, one STFT
// over the table, the ready crops of all streams and both passes as ONE list through run_crop_chunks in parts of `bs` (one gather, one
// network pass and one head launch per part: the head scatters every item into its own stream's mask ring through a pointer table),
// one masked iSTFT per stem over the table.  Per call: inputs in, outputs out, one drain.
// pcm: the parts' `wave` are sample bytes (channels, fmt per part).  They are staged as bytes, a PcmIn table rides beside the StreamSeg table
// of every round, and the PCM form of the stream STFT reads the block through it; everything behind the STFT is the same.
void Model::stream_run(std::vector<StreamPart>& parts, int bs, bool on_dev, bool out_on_dev, bool pcm) {
    const int np = (int)parts.size();
    const int cropsize = parts[0].S->cropsize, roi = parts[0].S->roi, bins = output_bin, E = is_complex ? 2 : 1;
    size_t list_cap = 0;
    bool any_crops = false;                          // (a MEASURE stream runs no crops: no gather buffer for it)
    for (const StreamPart& p : parts) { list_cap += (size_t)2 * (p.S->RM / roi); any_crops = any_crops || !p.S->measure; }

    DeviceGuard dev_guard(device);
    // ---- the staging arena: carved twice, first dry for its size
    const size_t crop_f = (size_t)nin * max_bin * cropsize;
    StreamSeg* seg_d = nullptr;
    PcmIn* pin_d = nullptr;
    auto frame_bytes = [](const StreamPart& p) { return (size_t)p.channels * pcm_sample_bytes(p.fmt); };
    unsigned long long* list_d = nullptr;            // per round: the crop list (int2 per crop), one mask destination per crop, its row pitch
    float* gather = nullptr;
    auto carve = [&](Arena& A) {
        seg_d = static_cast<StreamSeg*>(A.alloc(sizeof(StreamSeg) * np));
        if (pcm) pin_d = static_cast<PcmIn*>(A.alloc(sizeof(PcmIn) * np));
        list_d = static_cast<unsigned long long*>(A.alloc(24 * list_cap));
        if (any_crops) gather = A.allocf((size_t)bs * crop_f + 4096);
        for (StreamPart& p : parts) {
            // (bytes are staged as bytes, rounded up so that pcm_load24's aligned word reads stay inside the allocation)
            if (pcm) p.stage_in = (!on_dev && p.n > 0) ? A.allocf(((size_t)p.n * frame_bytes(p) + 3) / 4 + 1) : nullptr;
            else p.stage_in = (!on_dev && p.n > 0) ? A.allocf((size_t)2 * p.n) : nullptr;
            p.stage_y = (!out_on_dev && p.need > 0) ? A.allocf((size_t)2 * p.need + 4) : nullptr;
            p.stage_v = (!out_on_dev && p.need > 0) ? A.allocf((size_t)2 * p.need + 4) : nullptr;
        }
    };
    Arena dry_a;
    dry_a.dry = true;
    carve(dry_a);
    ensure_io(dry_a.peak + 65536);
    io.reset();
    carve(io);
    for (StreamPart& p : parts) p.S->broken = true;  // until the call has gone through: a failure half way leaves the rings undefined
    // host copies of what the rounds send to the device, alive until the call has drained
    std::deque<std::vector<StreamSeg>> segs_h;
    std::deque<std::vector<PcmIn>> pins_h;
    std::deque<std::vector<unsigned long long>> lists_h;
    try {
        for (StreamPart& p : parts) {
            if (p.stage_in)
                VR_HIP(hipMemcpyAsync(p.stage_in, p.wave, pcm ? (size_t)p.n * frame_bytes(p) : (size_t)2 * p.n * sizeof(float), hipMemcpyHostToDevice, stream));
            p.at = 0; p.flush_done = false;
            p.o = StreamStepIO{};
            p.o.blk_pitch = p.n;
            p.o.y = out_on_dev ? p.y : p.stage_y; p.o.v = out_on_dev ? p.v : p.stage_v;
            p.o.out_pitch = out_on_dev ? p.capacity : p.need;
        }
        std::vector<int> live;                       // the parts that take a step in this round
        std::vector<StreamStepPlan> plans;
        std::vector<StreamCrop> list;
        for (;;) {
            live.clear(); plans.clear(); list.clear();
            for (int i = 0; i < np; ++i) {
                StreamPart& p = parts[i];
                StreamState& S = *p.S;
                // the next block of this part: at most chunk_frames new frames; a running normaliser's block also ends with the
                // window of its next crop, so that crop i's statistics cover exactly the frames below its window's end; the flush
                // step takes no samples and comes last
                const bool final = p.at >= p.n;
                if (final && (!p.flush || p.flush_done)) continue;
                long long take = std::min((long long)S.chunk_frames * hop, p.n - p.at);
                if (S.running) take = std::min(take, ((S.crops[0] + 1) * S.roi + offset) * (long long)hop - S.samples);
                const float* src = p.n > 0 ? (on_dev ? p.wave : p.stage_in) : nullptr;
                p.o.blk = final ? src : src + p.at; p.o.blk_n = take;
                if (pcm) {                            // the step's bytes begin at frame p.at: any byte address for PCM24
                    p.o.pcm = PcmIn{(final || !src) ? nullptr : reinterpret_cast<const uint8_t*>(src) + (size_t)p.at * frame_bytes(p), p.channels, p.fmt};
                    p.o.blk = nullptr;
                }
                p.at += take;
                p.flush_done = final;
                const int entry = (int)live.size();
                plans.push_back(stream_step_plan(S, p.o, final));
                stream_step_crops(S, plans.back(), entry, list);
                live.push_back(i);
                if (final) S.flushed = true;
            }
            if (live.empty()) break;
            const int ne = (int)live.size();
            segs_h.emplace_back((size_t)ne);
            int max_new = 0, max_seg = 0, max_post = 0;
            double sum_new = 0, sum_seg = 0, sum_blk = 0, sum_post = 0;
            bool any_tta = false, post_walk = false;
            for (int e = 0; e < ne; ++e) {
                segs_h.back()[e] = plans[e].seg;
                max_new = std::max(max_new, plans[e].new_frames); sum_new += plans[e].new_frames;
                max_seg = std::max(max_seg, plans[e].segments); sum_seg += plans[e].segments;
                max_post = std::max(max_post, plans[e].post_frames); sum_post += plans[e].post_frames;
                post_walk = post_walk || plans[e].post_walk;
                sum_blk += (double)parts[live[e]].o.blk_n;
                any_tta = any_tta || parts[live[e]].S->tta;
            }
            VR_HIP(hipMemcpyAsync(seg_d, segs_h.back().data(), sizeof(StreamSeg) * ne, hipMemcpyHostToDevice, stream));
            if (pcm) {
                pins_h.emplace_back((size_t)ne);
                double blk_bytes = 0;
                for (int e = 0; e < ne; ++e) {
                    pins_h.back()[e] = parts[live[e]].o.pcm;
                    blk_bytes += (double)parts[live[e]].o.blk_n * (double)frame_bytes(parts[live[e]]);
                }
                VR_HIP(hipMemcpyAsync(pin_d, pins_h.back().data(), sizeof(PcmIn) * ne, hipMemcpyHostToDevice, stream));
                launch_stft_stream(plan, seg_d, ne, max_new, sum_blk, sum_new, stream, pin_d, blk_bytes);
            } else
                launch_stft_stream(plan, seg_d, ne, max_new, sum_blk, sum_new, stream);
            for (int e = 0; e < ne; ++e) {           // the statistics of a MEASURE / running stream, and a running stream's 1 / c before its crops
                const StreamState& S = *parts[live[e]].S;
                if (plans[e].new_frames > 0 && (S.measure || S.running))
                    launch_stream_stats(seg_d + e, bins, plans[e].new_frames, reinterpret_cast<unsigned long long*>(S.stats) + 2, stream);
                if (S.running && plans[e].p.crops[0] > S.crops[0]) {
                    if (is_complex) launch_coef_complex(S.stats, 2 * bins, 0, reinterpret_cast<float2*>(S.aff), stream);
                    else launch_coef_affine(S.stats, 2 * bins, 0, S.aff, stream);
                }
            }
            // ---- the crops of all streams that became ready: stream-major, pass 0 then pass 1 inside a stream, in device batches of bs
            if (!list.empty()) {
                const int nc = (int)list.size();
                VR_CHECK((size_t)nc <= list_cap, -4, "stream crop list overflow (planning bug)");
                lists_h.emplace_back((size_t)2 * nc + ((size_t)nc + 1) / 2);
                std::vector<unsigned long long>& lh = lists_h.back();
                for (int c = 0; c < nc; ++c) {
                    const StreamCrop& cr = list[c];
                    const StreamState& S = *parts[live[cr.entry]].S;
                    const int2 at = make_int2(cr.entry, (int)(cr.idx * roi - offset - (cr.pass ? roi / 2 : 0)));
                    memcpy(&lh[c], &at, 8);
                    // (RM is a multiple of roi: the roi columns of a crop never wrap inside the ring)
                    lh[(size_t)nc + c] = (unsigned long long)reinterpret_cast<uintptr_t>(S.mask[cr.pass] + (size_t)E * (cr.idx * roi % S.RM));
                    reinterpret_cast<int*>(&lh[(size_t)2 * nc])[c] = S.RM;
                }
                VR_HIP(hipMemcpyAsync(list_d, lh.data(), lh.size() * 8, hipMemcpyHostToDevice, stream));
                const int2* crops_d = reinterpret_cast<const int2*>(list_d);
                float* const* items_d = reinterpret_cast<float* const*>(list_d + nc);
                const int* pitch_d = reinterpret_cast<const int*>(list_d + 2 * (size_t)nc);
                fold_eval_affines();                // before planning, as in forward_api
                plan_and_reserve(bs, cropsize, 0);
                auto run_crops = [&](int first, int count) {
                    float* dense = gather + (size_t)(first % bs) * crop_f;
                    launch_stream_gather(seg_d, crops_d + first, count, is_complex, bins, max_bin, cropsize, dense, stream);
                    HeadDst d{};
                    d.items = items_d + first; d.item_pitch = pitch_d + first;
                    run_dense_crops(dense, count, cropsize, d);
                };
                run_crop_chunks(nc, bs, run_crops);
            }
            // --postprocess streams: the minima of the masks that became final, then the walk that turns them into blend weights
            if (max_post > 0 || post_walk) launch_stream_post(seg_d, ne, max_post, sum_post, post_walk, is_complex, any_tta, bins, stream);
            for (int which = 0; which < 2; ++which)     // (no launch when no entry has a final segment)
                launch_istft_stream(plan, seg_d, ne, max_seg, sum_seg, is_complex, any_tta, which, stream, parts[0].S->pcm16);
            for (int e = 0; e < ne; ++e) stream_step_commit(*parts[live[e]].S, parts[live[e]].o, plans[e]);
        }
        for (StreamPart& p : parts) {
            VR_CHECK(p.o.out_off == p.need, -4, "stream schedule mismatch (planning bug)");
            if (p.flush && p.S->measure) {
                p.st.resize((size_t)2 * 2 * bins);
                VR_HIP(hipMemcpyAsync(p.st.data(), reinterpret_cast<unsigned long long*>(p.S->stats) + 2, p.st.size() * 8, hipMemcpyDeviceToHost, stream));
            }
            if (!out_on_dev && p.need > 0 && p.S->pcm16) {      // interleaved int16: `need` frames of 4 bytes, one piece
                VR_HIP(hipMemcpyAsync(p.y, p.stage_y, (size_t)p.need * 4, hipMemcpyDeviceToHost, stream));
                VR_HIP(hipMemcpyAsync(p.v, p.stage_v, (size_t)p.need * 4, hipMemcpyDeviceToHost, stream));
            } else if (!out_on_dev && p.need > 0) {
                VR_HIP(hipMemcpy2DAsync(p.y, (size_t)p.capacity * 4, p.stage_y, (size_t)p.need * 4, (size_t)p.need * 4, 2, hipMemcpyDeviceToHost, stream));
                VR_HIP(hipMemcpy2DAsync(p.v, (size_t)p.capacity * 4, p.stage_v, (size_t)p.need * 4, (size_t)p.need * 4, 2, hipMemcpyDeviceToHost, stream));
            }
        }
        VR_HIP(hipStreamSynchronize(stream));
    } catch (...) {
        hipStreamSynchronize(stream);               // the host copies above must outlive every copy that is still in flight
        throw;
    }
    for (StreamPart& p : parts) {
        StreamState& S = *p.S;
        if (p.flush && S.measure) {
            unsigned mxb = 0;
            unsigned long long key = ((unsigned long long)host_ord32(0.f) << 32) | host_ord32(0.f);
            for (int r = 0; r < 2 * bins; ++r) {
                mxb = std::max(mxb, (unsigned)p.st[2 * r]);         // non-negative floats order like their bit patterns
                key = std::max(key, p.st[2 * r + 1]);
            }
            if (S.tta) {
                S.coef[0] = host_unord32((unsigned)(key >> 32)); S.coef[1] = host_unord32((unsigned)(key & 0xffffffffu));
            } else {
                float m;
                memcpy(&m, &mxb, 4);
                S.coef[0] = m; S.coef[1] = 0.0;
            }
        }
        S.broken = false;
    }
}

void Model::stream_push(StreamState& S, const float* wave, bool on_dev, long long n, bool flush, float* y, float* v, bool out_on_dev,
                        long long capacity, long long* n_out, int channels, int fmt) {
    VR_CHECK(!training, -2, "a stream runs in eval mode (inference.py:52); call vr_set_mode(h, 0) first");
    if (fmt) {
        VR_CHECK(n >= 0 && (n == 0 || wave), -2, "null or negative input");
        check_pcm(on_dev && n > 0 ? wave : nullptr, channels, fmt, "");
    }
    std::vector<StreamPart> parts(1);
    StreamPart& p = parts[0];
    p.S = &S; p.wave = wave; p.n = n; p.flush = flush; p.y = y; p.v = v; p.capacity = capacity; p.channels = channels; p.fmt = fmt;
    p.need = stream_check(S, "", wave, n, flush, y, v, out_on_dev, capacity);
    if (n_out) *n_out = 0;
    if (n == 0 && !flush) return;
    stream_run(parts, S.bs, on_dev, out_on_dev, fmt != 0);
    if (n_out) *n_out = p.need;
}

// vr_stream_push_many: stream k gets n_in[k] more samples and, flush[k], its end.  With one stream it is stream_push.
void Model::stream_push_many(int n_streams, StreamState* const* Sv, const float* const* wave, bool on_dev, const long long* n_in, const int* flush,
                             int batchsize, float* const* y, float* const* v, bool out_on_dev, const long long* capacity, long long* n_out,
                             const int* channels, const int* fmt) {
    // ---- arguments and the schedule of this call: nothing here touches the device or a stream
    VR_CHECK(n_streams >= 1, -2, "n_streams must be positive");
    VR_CHECK(Sv && n_in && (!fmt || channels), -2, "null table");
    VR_CHECK(!training, -2, "a stream runs in eval mode (inference.py:52); call vr_set_mode(h, 0) first");
    std::vector<StreamPart> parts;
    std::vector<int> part_k;
    int bs = batchsize;
    for (int k = 0; k < n_streams; ++k) {
        const std::string who = "stream " + std::to_string(k) + ": ";
        VR_CHECK(Sv[k], -2, who + "null stream (closed?)");
        StreamState& S = *Sv[k];
        for (int j = 0; j < k; ++j) VR_CHECK(Sv[j] != Sv[k], -2, who + "the same stream as stream " + std::to_string(j));
        VR_CHECK(S.cropsize == Sv[0]->cropsize, -2, who + "cropsize " + std::to_string(S.cropsize) + " differs from stream 0's " +
                                                        std::to_string(Sv[0]->cropsize) + ": the streams of one call share device batches");
        VR_CHECK(!S.measure, -2, who + "a VR_STREAM_MEASURE stream is not taken by vr_stream_push_many: use vr_stream_push");
        VR_CHECK(!S.running, -2, who + "a running-normaliser stream (coef 0) is not taken by vr_stream_push_many: its steps are cut per crop, "
                                       "use vr_stream_push");
        VR_CHECK(S.pcm16 == Sv[0]->pcm16, -2, who + "VR_STREAM_PCM16_OUT differs from stream 0's: the streams of one call share the masked iSTFT "
                                                   "launch, which stores one sample format");
        StreamPart p{};
        p.S = &S; p.wave = wave ? wave[k] : nullptr; p.n = n_in[k]; p.flush = flush && flush[k];
        p.y = y ? y[k] : nullptr; p.v = v ? v[k] : nullptr; p.capacity = capacity ? capacity[k] : 0;
        if (fmt) {
            VR_CHECK(p.n >= 0 && (p.n == 0 || p.wave), -2, who + "null or negative input");
            check_pcm(on_dev && p.n > 0 ? p.wave : nullptr, channels[k], fmt[k], who);
            p.channels = channels[k]; p.fmt = fmt[k];
        }
        p.need = stream_check(S, who, p.wave, p.n, p.flush, p.y, p.v, out_on_dev, p.capacity);
        if (batchsize <= 0) bs = std::max(bs, S.bs);
        if (p.n == 0 && !p.flush) continue;          // untouched
        parts.push_back(p);
        part_k.push_back(k);
    }
    if (n_out) for (int k = 0; k < n_streams; ++k) n_out[k] = 0;
    if (parts.empty()) return;
    stream_run(parts, bs, on_dev, out_on_dev, fmt != nullptr);
    if (n_out) for (size_t i = 0; i < parts.size(); ++i) n_out[part_k[i]] = parts[i].need;
}

// =====================================================================================================
// unit-test hooks: the weight forms of a single conv launch
// =====================================================================================================
void Model::debug_weight_forms(const float* dw_, int Cin, int KS, int stride, int dh, int dw, int CoutPad, int Win, bool want_wino,
                               ConvArgs& a, LocalConv& lc) {
    Conv& L = lc.L;
    L.name = "debug"; L.Cin = Cin; L.Cout = L.CoutPad = CoutPad; L.KS = KS;    // (no forward form depends on Cout)
    L.stride = stride; L.dh = dh; L.dw = dw;
    L.cls = form_class(KS, stride, dh, dw, true);            // (the hook takes any 1x1 stride-1 conv for a conv_x3d layer)
    lc.P.dev = const_cast<float*>(dw_);
    // Where the hook differs from the handle: a stride-2 layer gets its planes under option conv_x3s only (and with or without the
    // flag -- no other form exists for it), every other layer its forms only when asked; the bf16 planes of U exist for every plain
    // layer in mfma_mode 2.
    const bool x3dl = mfma_mode == 3 && (L.cls == FC_X3D || L.cls == FC_S2);
    if (want_wino && !x3dl) VR_CHECK(L.cls == FC_PLAIN3, -2, "Winograd weights exist for 3x3 stride-1 convs only");
    const bool made = L.cls == FC_S2 ? x3s_mode != 0 : want_wino;
    const std::vector<Conv*> one{&L};
    for (FormId f : {F_WINO, F_WINO6, F_X3W}) {
        const FormSpec sp = form_spec(f, L, mfma_mode, W6_ALL);
        if (!(made && sp.held && sp.live)) continue;
        hold_form(f, one, W6_ALL, lc.store);
        fill_form(f, one, W6_ALL, lc.store, true);
    }
    FormSelect sel = form_select();
    sel.training = false;                                    // (the hook's launch reads what was made for it, as an eval launch does)
    select_fwd_forms(a, L.forms, sel, Win, stride);
}

// =====================================================================================================
// unit-test hook: one conv through the MFMA kernel with a single dense source
// =====================================================================================================
void Model::debug_conv(const float* x, int N, int Cin, int H, int W, const float* w_oihw, int Cout, int KS, int stride,
                       int dh, int dw, int flags, const float* aff, float slope, const float* bias, float* out,
                       float* stats_out) {
    DeviceGuard dev_guard(device);
    // flags: bit 0 = fused x2 upsample; bit 1 = give the launch Winograd-domain weights (conv_wino.hip);
    //        bit 2 = `aff`/`slope` describe the EPILOGUE ([Cout][2] folded BatchNorm + activation, eval mode)
    const int up = flags & 1;
    const bool want_wino = (flags & 2) != 0, epi = (flags & 4) != 0;
    const int KK = KS * KS, CoutPad = round_up(Cout, 32);
    const int Hin = up ? 2 * H : H, Win = up ? 2 * W : W;
    const int pad_h = KS == 1 ? 0 : dh, pad_w = KS == 1 ? 0 : dw;
    const int Hout = (Hin + 2 * pad_h - dh * (KS - 1) - 1) / stride + 1;
    const int Wout = (Win + 2 * pad_w - dw * (KS - 1) - 1) / stride + 1;
    std::vector<float> wk((size_t)Cin * KK * CoutPad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < KK; ++k) wk[((size_t)ci * KK + k) * CoutPad + co] = w_oihw[((size_t)co * Cin + ci) * KK + k];
    float *dx, *dw_, *dout, *daff = nullptr, *dbias = nullptr, *dpart = nullptr;
    const size_t xin = (size_t)N * Cin * H * W, xout = (size_t)N * Cout * Hout * Wout;
    VR_HIP(hipMalloc(&dx, xin * 4)); VR_HIP(hipMalloc(&dw_, wk.size() * 4)); VR_HIP(hipMalloc(&dout, xout * 4));
    VR_HIP(hipMemcpy(dx, x, xin * 4, hipMemcpyHostToDevice));
    VR_HIP(hipMemcpy(dw_, wk.data(), wk.size() * 4, hipMemcpyHostToDevice));
    const size_t naff = epi ? Cout : Cin;
    if (aff) { VR_HIP(hipMalloc(&daff, naff * 8)); VR_HIP(hipMemcpy(daff, aff, naff * 8, hipMemcpyHostToDevice)); }
    if (bias) { VR_HIP(hipMalloc(&dbias, (size_t)Cout * 4)); VR_HIP(hipMemcpy(dbias, bias, (size_t)Cout * 4, hipMemcpyHostToDevice)); }
    Tensor t;
    t.p = dx; t.N = N; t.C = Cin; t.H = H; t.W = W; t.sH = W; t.sC = (long long)H * W; t.sN = t.sC * Cin;
    if (!epi) { t.aff0 = daff; t.slope = slope; }
    ConvArgs a{};
    a.nsrc = 1; a.src[0] = make_src(t, up != 0, 0); a.c1 = a.c2 = Cin; a.Cin = Cin;
    a.w = dw_; a.bias = dbias; a.Cout = Cout; a.CoutPad = CoutPad;
    if (epi && daff) { a.epi = daff; a.epi_slope = slope; }
    a.bf16 = mfma_mode;
    LocalConv wf;
    debug_weight_forms(dw_, Cin, KS, stride, dh, dw, CoutPad, Win, want_wino, a, wf);
    a.dst[0] = ConvDst{dout, (long long)Hout * Wout * Cout, (long long)Hout * Wout, (long long)Wout, 0};
    a.d1 = a.d2 = 1 << 30;
    a.N = N; a.Hout = Hout; a.Wout = Wout; a.Hin = Hin; a.Win = Win; a.pad_h = pad_h; a.pad_w = pad_w;
    const ConvShape shp{KS, stride, dh, dw};
    size_t npt = 0;
    if (stats_out) { npt = conv_part_count(a, shp); VR_HIP(hipMalloc(&dpart, npt * Cout * 8)); a.part = dpart; }
    launch_conv(a, shp, stream);
    VR_HIP(hipStreamSynchronize(stream));
    VR_HIP(hipMemcpy(out, dout, xout * 4, hipMemcpyDeviceToHost));
    if (stats_out) {
        std::vector<float> part(npt * Cout * 2);
        VR_HIP(hipMemcpy(part.data(), dpart, part.size() * 4, hipMemcpyDeviceToHost));
        for (int c = 0; c < Cout; ++c) {
            double s1 = 0, s2 = 0;
            for (size_t i = 0; i < npt; ++i) { s1 += part[(i * Cout + c) * 2]; s2 += part[(i * Cout + c) * 2 + 1]; }
            stats_out[2 * c] = (float)s1; stats_out[2 * c + 1] = (float)s2;
        }
    }
    hipFree(dx); hipFree(dw_); hipFree(dout); hipFree(daff); hipFree(dbias); hipFree(dpart);
}

}  // namespace vr
