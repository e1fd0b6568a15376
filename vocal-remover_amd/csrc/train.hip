// Training executor: forward in train mode (model.hip) records a tape; this file walks it backwards
// (train.py:81-96: loss = L1(mask*X, y); (loss/accumulation_steps).backward(); optimizer.step()).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "model.h"
#include "pcm.h"

namespace vr {

ConvSrc make_src(const Tensor& t, bool up, int bcastH);

static inline int round_up32(int v) { return (v + 31) / 32 * 32; }

template <class F>
void Model::for_each_conv(F&& f) {
    for (int i = 0; i < 5; ++i) {
        BaseNetL& B = nets_[i];
        f(B.enc1);
        for (int j = 0; j < 4; ++j) { f(B.enc_a[j]); f(B.enc_b[j]); }
        f(B.aspp_pool); f(B.aspp_c2);
        for (int j = 0; j < 3; ++j) f(B.aspp_d[j]);
        f(B.aspp_bott);
        for (int j = 0; j < 4; ++j) f(B.dec[j]);
        f(B.lstm.proj); f(B.lstm.dense);
    }
    f(tail1); f(tail2);
}

const std::vector<Conv*>& Model::conv_layers() {
    if (convs_.empty()) for_each_conv([&](Conv& L) { convs_.push_back(&L); });
    return convs_;
}

void Model::ensure_train_state() {
    if (g_arena) return;
    VR_HIP(hipMalloc(&g_arena, p_floats * sizeof(float)));
    VR_HIP(hipMalloc(&m_arena, p_floats * sizeof(float)));
    VR_HIP(hipMalloc(&v_arena, p_floats * sizeof(float)));
    VR_HIP(hipMemset(g_arena, 0, p_floats * sizeof(float)));
    VR_HIP(hipMemset(m_arena, 0, p_floats * sizeof(float)));
    VR_HIP(hipMemset(v_arena, 0, p_floats * sizeof(float)));
    // flipped + transposed copies of the conv weights for the data-gradient launches, and the four parity-class weight tensors of each
    // stride-2 3x3 conv (both refreshed once per step)
    hold_form(F_WT, conv_layers(), W6_PAD64, form_store);
    hold_form(F_S2W, conv_layers(), W6_PAD64, form_store);
}

void Model::zero_grad_api() {
    DeviceGuard dev_guard(device);
    ensure_train_state();
    prof_memset_async(g_arena, 0, p_floats * sizeof(float), stream);
    VR_HIP(hipStreamSynchronize(stream));
}

void Model::grad_arena(float** ptr, int64_t* numel) {
    DeviceGuard dev_guard(device);
    ensure_train_state();
    *ptr = g_arena;
    *numel = (int64_t)p_floats;
}

void Model::set_dropout(int mode, unsigned long long seed, const float* masks, int B) {
    VR_CHECK(mode >= 0 && mode <= 2, -2, "dropout mode must be 0 (off), 1 (native RNG) or 2 (injected)");
    dropout_mode = mode;
    dropout_seed = seed;
    dropout_host.clear();
    if (mode == 2) {
        VR_CHECK(masks && B > 0, -2, "injected dropout needs masks [5][B][8*nout]");
        dropout_host.assign(masks, masks + (size_t)5 * B * 8 * nout);
    }
}

// nn.Dropout2d(0.1) keep-masks for one train-mode forward (lib/layers.py:90: the five ASPP outputs), [5][B][8*nout]
// holding 0 or 1/0.9.  Mode 1 draws them on the device from a counter-based generator keyed on (seed, number of
// train-mode forwards so far, element): every forward -- each micro-batch of an accumulation window too -- gets a
// fresh draw, as torch does, and nothing restarts when the optimizer is re-created.
__global__ void dropout_mask_kernel(float* __restrict__ m, long long n, unsigned long long seed, unsigned long long call) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long x = seed + 0x9E3779B97F4A7C15ull * (call + 1) + 0xD1B54A32D192ED03ull * (unsigned long long)(i + 1);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;            // splitmix64 finalizer
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    const float u = (float)(x >> 40) * (1.f / 16777216.f);
    m[i] = (u >= 0.1f) ? (1.f / 0.9f) : 0.f;
}

void Model::prepare_dropout(int B) {
    dropout_dev = nullptr;
    train_calls += 1;
    if (dropout_mode == 0) return;
    const size_t n = (size_t)5 * B * 8 * nout;
    if (n > dropout_cap) {
        VR_HIP(hipStreamSynchronize(stream));
        if (dropout_buf) VR_HIP(hipFree(dropout_buf));
        dropout_buf = nullptr; dropout_cap = 0;
        VR_HIP(hipMalloc(&dropout_buf, n * sizeof(float)));
        dropout_cap = n;
    }
    if (dropout_mode == 2) {
        VR_CHECK(dropout_host.size() == n, -2, "injected dropout masks were given for a different batch size");
        VR_HIP(hipMemcpyAsync(dropout_buf, dropout_host.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
    } else {
        VR_LAUNCH(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dropout_buf, (long long)n,
                           dropout_seed, train_calls);
        VR_HIP(hipGetLastError());
    }
    dropout_dev = dropout_buf;
}

// BatchNorm backward of a conv record: G -> dz in place, d(gamma), d(beta) into the gradient arena.
void Model::bwd_bn_of(const Tensor& out, Conv& L) {
    BN* b = L.bn;
    BnBwdArgs a{};
    a.g = out.g; a.z = out.p; a.N = out.N; a.C = out.C; a.H = out.H; a.W = out.W;
    a.sN = out.sN; a.sC = out.sC; a.sH = out.sH;
    a.aff = b->affine; a.aff_bcast = b->bcast ? 1 : 0; a.slope = L.slope; a.post = out.post;
    a.gamma = b->w->dev; a.save_mean = b->save_mean; a.save_invstd = b->save_invstd;
    a.dgamma = dry ? nullptr : grad_of(b->w); a.dbeta = dry ? nullptr : grad_of(b->b);
    a.acc_grads = 1;
    a.coef = ws.allocf((size_t)out.C * 3);
    a.part = ws.allocf((size_t)bn_bwd_chunks(a) * out.C * 2);
    if (!dry && g_first(out.g))            // no consumer wrote a gradient into this tensor (does not happen in this net): it is zero
        prof_memset_async(out.g, 0, (size_t)out.N * out.C * out.H * out.W * sizeof(float), stream);
    if (!dry) launch_bn_bwd(a, stream);
}

void Model::bwd_conv(TapeRec& r) {
    Conv& L = *r.L;
    const Tensor& out = r.out;
    const int N = r.N;
    // 1. gradient at the raw conv output
    if (L.bn) bwd_bn_of(out, L);
    // (no BatchNorm: the only such convs -- LSTM input projection -- have identity activation: dz = G)
    // 2. bias gradient (Linear bias): channel sums of dz laid out [N][C][W]
    if (r.bias_param && !dry) launch_channel_sum(out.g, N, out.C, out.W, grad_of(r.bias_param), 1, stream);
    // 3. weight gradient
    ConvArgs f;
    build_fwd_args(L, r.srcs, N, r.batch_as_h, f);
    const ConvShape shp{L.KS, L.stride, L.dh, L.dw};
    {
        WgradArgs w{};
        w.in = f;
        w.dz = out.g;
        if (r.batch_as_h) { w.zN = 0; w.zC = out.sC; w.zH = out.sN; }
        else { w.zN = out.sN; w.zC = out.sC; w.zH = out.sH; }
        w.Cout = L.Cout; w.CoutPad = L.CoutPad;
        w.allow_wino = train_wino ? 1 : 0;
        w.bf16 = mfma_mode;                      // 1: bf16 MFMA operands (wgrad_wino / wgrad_gemm); 2: split-bf16 products (wgrad_x3.hip)
        w.part = ws.allocf(wgrad_scratch_floats(w, shp));
        if (!dry) {
            // The weight gradient is off the critical path (dz -> data gradient -> previous layer): it runs on the
            // side stream beside the data-gradient / BatchNorm-backward chain, so the element-wise passes and the
            // tails of one stream's kernels fill the other's bubbles.  backward() joins before returning.
            static const bool overlap = !getenv("VR_NO_WGRAD_OVERLAP");
            hipStream_t wst = stream;
            if (overlap && !serial && !profiling && side_stream) {
                VR_HIP(hipEventRecord(ev_fork, stream));          // dz (and every forward tensor) is ready here
                VR_HIP(hipStreamWaitEvent(side_stream, ev_fork, 0));
                wst = side_stream;
                wgrad_on_side = true;
            }
            record_begin(0, 2.0 * N * (double)(r.batch_as_h ? 1 : f.Hout) * f.Wout * (double)L.Cout * L.Cin * L.KS * L.KS);
            record_note(conv_alg_bytes(L, f, N, r.batch_as_h), ("wgrad " + L.name).c_str());
            launch_wgrad(w, shp, grad_of(L.w), 1, wst);
            record_end();
        }
    }
    // 4. data gradient, split back to the sources of the virtual concat
    bwd_conv_dgrad(r, f);
}

// Step 4 of bwd_conv: the data gradient of one conv record, split back to the sources of the virtual concat (f: the record's forward
// launch, build_fwd_args).  Returns the path it took (DgradPath; DG_NONE in a dry pass or when no source wants a gradient).
int Model::bwd_conv_dgrad(TapeRec& r, const ConvArgs& f) {
    Conv& L = *r.L;
    const Tensor& out = r.out;
    const int N = r.N;
    bool any = false;
    for (auto& sp : r.srcs) any = any || sp.t.g != nullptr;
    if (!any) return DG_NONE;
    ConvArgs d{};
    Tensor dzt = out;                       // dz as a plain source
    dzt.p = out.g; dzt.aff0 = dzt.aff1 = nullptr; dzt.slope = 1.f; dzt.post = nullptr; dzt.hsplit = 1 << 30;
    d.nsrc = 1;
    d.src[0] = make_src(dzt, false, 0);
    if (r.batch_as_h) { d.src[0].sH = d.src[0].sN; d.src[0].sN = 0; d.src[0].H = N; }
    d.src[0].zins = (L.stride == 2) ? 1 : 0;
    d.c1 = d.c2 = L.Cout; d.Cin = L.Cout;
    select_dgrad_forms(d, L.forms, L.cls, form_select(), f.Win);
    d.bias = nullptr;
    d.bf16 = mfma_mode;
    d.Cout = L.Cin; d.CoutPad = round_up32(L.Cin);
    d.N = f.N; d.Hin = f.Hin; d.Win = f.Win; d.Hout = f.Hin; d.Wout = f.Win;
    d.pad_h = (L.KS == 1) ? 0 : L.dh; d.pad_w = (L.KS == 1) ? 0 : L.dw;
    struct Post { int kind; float* tmp; const SrcSpec* sp; };
    std::vector<Post> posts;
    int cbase = 0;
    for (size_t i = 0; i < r.srcs.size(); ++i) {
        const SrcSpec& sp = r.srcs[i];
        const Tensor& t = sp.t;
        ConvDst ds{};
        if (!t.g) {
            ds.p = nullptr;
        } else if (sp.up || sp.bcastH) {
            const size_t n = (size_t)N * t.C * f.Hin * f.Win;
            float* tmp = ws.allocf(n);
            ds = ConvDst{tmp, (long long)t.C * f.Hin * f.Win, (long long)f.Hin * f.Win, (long long)f.Win, 0};
            posts.push_back(Post{sp.up ? 1 : 2, tmp, &sp});
        } else if (r.batch_as_h) {
            ds = ConvDst{t.g, 0, t.sC, t.sN, 1};
        } else {
            ds = ConvDst{t.g, t.sN, t.sC, t.sH, (!dry && g_first(t.g)) ? 0 : 1};      // the tensor's first backward writer stores
        }
        d.dst[i] = ds;
        cbase += t.C;
        if (i == 0) d.d1 = cbase;
        if (i == 1) d.d2 = cbase;
    }
    if (r.srcs.size() == 1) d.d1 = d.d2 = 1 << 30;
    if (r.srcs.size() == 2) d.d2 = 1 << 30;
    if (dry) return DG_NONE;
    // Stride-2 3x3: four parity-class stride-1 convs over dz (9 tap evaluations) instead of one conv over the
    // zero-inserted gradient (36), when the LDS-DMA kernel covers the shape.
    {
        static const bool s2_classes = !getenv("VR_NO_S2_CLASSES");
        const float* s2w = L.forms.f32(F_S2W);
        bool ok = s2_classes && L.stride == 2 && L.KS == 3 && s2w && posts.empty() && !r.batch_as_h;
        if (ok) {
            ConvArgs c = d;
            c.src[0].zins = 0;
            c.Hin = out.H; c.Win = out.W;
            const ConvShape cshp{3, 1, 1, 1};
            const size_t cls_stride = (size_t)L.Cout * 9 * round_up32(L.Cin);
            // all four classes in one launch (one staging of dz and of the nine live (class, tap) weight slices per chunk)
            {
                ConvArgs k = c;
                k.Hout = (f.Hin + 1) / 2; k.Wout = (f.Win + 1) / 2;
                k.w = s2w; k.wino = nullptr; k.wino6 = nullptr; k.x3w = nullptr;
                k.s2_cls_stride = (long long)cls_stride; k.s2_H = f.Hin; k.s2_W = f.Win;
                if (s2d_fused_eligible(k)) {
                    record_begin(0, 2.0 * N * (double)f.Hout * f.Wout * (double)L.Cout * L.Cin * L.KS * L.KS);
                    record_note(conv_alg_bytes(L, f, N, false), ("dgrad " + L.name).c_str());
                    launch_s2d_fused(k, stream);
                    record_end();
                    return DG_S2_FUSED;
                }
            }
            // Eligibility is decided for ALL four classes before the first launch: with an odd width the pw = 1 classes are one column
            // narrower than class 0 and may fall below the tap-masked kernel's 32 columns -- then nothing has been written yet and the
            // zero-insertion launch below computes the whole gradient.
            const int masks[2] = {1 << 1, (1 << 1) | (1 << 2)};          // live taps along one axis: parity 0 / 1
            ConvArgs cls_args[4];
            for (int cls = 0; cls < 4 && ok; ++cls) {
                const int ph = cls >> 1, pw = cls & 1;
                ConvArgs& k = cls_args[cls];
                k = c;
                k.Hout = (f.Hin - ph + 1) / 2; k.Wout = (f.Win - pw + 1) / 2;
                k.w = s2w + cls * cls_stride;
                k.wino = nullptr; k.wino6 = nullptr; k.x3w = nullptr;
                int tm = 0;
                for (int th = 0; th < 3; ++th)
                    for (int tw = 0; tw < 3; ++tw)
                        if (((masks[ph] >> th) & 1) && ((masks[pw] >> tw) & 1)) tm |= 1 << (th * 3 + tw);
                k.tapmask = tm;
                for (int i = 0; i < 3; ++i) {
                    if (!k.dst[i].p) continue;
                    k.dst[i].p += (long long)ph * k.dst[i].sH + pw;
                    k.dst[i].sH *= 2;
                    k.dst[i].wshift = 1;
                }
                if (k.Hout < 1 || k.Wout < 1 || conv_plan(k, cshp).k != CK_DMA) ok = false;
            }
            if (ok) {
                record_begin(0, 2.0 * N * (double)f.Hout * f.Wout * (double)L.Cout * L.Cin * L.KS * L.KS);
                record_note(conv_alg_bytes(L, f, N, false), ("dgrad " + L.name).c_str());
                for (int cls = 0; cls < 4; ++cls) launch_conv(cls_args[cls], cshp, stream);
                record_end();
                return DG_S2_CLASSES;
            }
        }
    }
    const ConvShape dshp{L.KS, 1, L.dh, L.dw};
    record_begin(0, 2.0 * N * (double)(r.batch_as_h ? 1 : f.Hout) * f.Wout * (double)L.Cout * L.Cin * L.KS * L.KS);
    record_note(conv_alg_bytes(L, f, N, r.batch_as_h), ("dgrad " + L.name).c_str());
    launch_conv(d, dshp, stream);
    record_end();
    for (auto& p : posts) {
        const Tensor& t = p.sp->t;
        if (p.kind == 1) launch_upsample_bwd(p.tmp, N, t.C, t.H, t.W, t.g, t.sN, t.sC, t.sH, g_first(t.g) ? 0 : 1, stream);
        else launch_sum_h(p.tmp, N, t.C, f.Hin, f.Win, t.g, stream);
    }
    return L.stride == 2 ? DG_S2_ZINS : DG_STRIDE1;
}

void Model::backward() {
    struct Join {                                      // the side stream's weight gradients must land before Adam
        Model* m;
        ~Join() {
            if (!m->wgrad_on_side) return;
            m->wgrad_on_side = false;
            hipEventRecord(m->ev_join, m->side_stream);
            hipStreamWaitEvent(m->stream, m->ev_join, 0);
        }
    } join{this};
    // The 107 wgrad_reduce launches of a step (~10 us each, launch-bound) become ONE launch behind the last weight gradient: launch_wgrad
    // only records what it would have summed (vr_common.h); flush_wgrad_sums() at the end of the tape launches the sum.
    static const bool defer_on = !getenv("VR_NO_WGRAD_DEFER");
    struct Unsink { ~Unsink() { wgrad_defer_to(nullptr); } } unsink;      // (also when a launch throws)
    wred_host.clear();
    if (defer_on && !dry) wgrad_defer_to(&wred_host);
    // Stages 1-2: the high-band records (chain 1) are independent of the low-band ones; in the reversed tape
    // they come first after stage 3, so they are enqueued on a second stream and the low chain follows on the main one.
    static const bool bwd_fork = !getenv("VR_NO_BWD_FORK");
    hipStream_t main_stream = stream;
    hipStream_t hi_stream = (bwd_fork && !serial && !dry && !profiling && !lanes.empty()) ? lanes[0].main : nullptr;
    int cur_chain = 0;
    bool hi_used = false;
    struct Restore {
        Model* m; hipStream_t s; hipStream_t hi; hipEvent_t ev; bool* used;
        ~Restore() {
            m->stream = s;
            if (*used) { hipEventRecord(ev, hi); hipStreamWaitEvent(s, ev, 0); }
        }
    } restore{this, main_stream, hi_stream, hi_stream ? lanes[0].done : nullptr, &hi_used};
    for (size_t k = tape.size(); k-- > 0;) {
        TapeRec& r = tape[k];
        if (hi_stream && r.chain != cur_chain) {
            if (r.chain == 1) {                    // entering the high chain: everything so far (stage 3) must be done
                VR_HIP(hipEventRecord(lanes[0].start, main_stream));
                VR_HIP(hipStreamWaitEvent(hi_stream, lanes[0].start, 0));
                stream = hi_stream;
                hi_used = true;
            } else {
                stream = main_stream;
            }
            cur_chain = r.chain;
        }
        switch (r.kind) {
        case TK_CONV:
            bwd_conv(r);
            break;
        case TK_AVGPOOL: {
            const Tensor& x5 = r.srcs[0].t;
            if (!dry && x5.g) launch_avgpool_bwd(r.out.g, x5.g, r.N, x5.C, x5.H, x5.W, x5.sN, x5.sC, x5.sH, g_first(x5.g) ? 0 : 1, stream);
            break;
        }
        case TK_SQUEEZE: {
            // 1x1 conv 2c->1 + BatchNorm(1) + ReLU (lib/layers.py:112): out is the 1-channel image z
            LSTMMod& M = *r.M;
            bwd_bn_of(r.out, M.squeeze);
            const Tensor& h = r.srcs[0].t;
            float* part = ws.allocf((size_t)thin_wgrad_blocks(h) * h.C);
            if (!dry) {
                launch_thin_wgrad(h, 1, r.out.g, part, grad_of(M.squeeze.w), 1, stream);
                launch_thin_dgrad(h, 1, M.squeeze.w->dev, r.out.g, h.g, g_first(h.g) ? 0 : 1, stream);
            }
            break;
        }
        case TK_LSTM: {
            LSTMMod& M = *r.M;
            const int H = M.hid, G = 4 * H, T = r.out.W, N = r.N;
            float* wpart = ws.allocf(lstm_whh_grad_scratch_floats(N, H));
            if (!dry) {
                launch_bilstm_bwd(r.out.g, r.save, M.whh_f->dev, M.whh_r->dev, r.aux.g, N, T, H, stream);
                launch_lstm_whh_grad(r.aux.g, r.out.p, grad_of(M.whh_f), grad_of(M.whh_r), N, T, H, 1, wpart, stream);
                // b_ih and b_hh enter the gates as a sum: both receive the channel sums of dgx
                float* tmp = ws.allocf((size_t)2 * G);
                launch_channel_sum(r.aux.g, N, 2 * G, T, tmp, 0, stream);
                launch_add(grad_of(M.b_ih_f), tmp, grad_of(M.b_ih_f), G, stream);
                launch_add(grad_of(M.b_hh_f), tmp, grad_of(M.b_hh_f), G, stream);
                launch_add(grad_of(M.b_ih_r), tmp + G, grad_of(M.b_ih_r), G, stream);
                launch_add(grad_of(M.b_hh_r), tmp + G, grad_of(M.b_hh_r), G, stream);
            } else {
                ws.allocf((size_t)2 * G);
            }
            break;
        }
        default:
            break;
        }
    }
    wgrad_defer_to(nullptr);
    flush_wgrad_sums();
}

// ONE launch for every deferred weight-gradient slab sum of this backward pass, behind the last weight gradient on its stream
void Model::flush_wgrad_sums() {
    if (wred_host.empty()) return;
    long long blocks = 0;
    const int vec = wgrad_reduce_vec(wred_host.data(), (int)wred_host.size());
    for (WgReduceDesc& d : wred_host) { d.blk0 = blocks; blocks += (d.n / vec + 63) / 64; }
    const size_t bytes = wred_host.size() * sizeof(WgReduceDesc);
    hipStream_t st = wgrad_on_side ? side_stream : stream;
    if (wred_cap < wred_host.size()) {
        if (wred_dev) { VR_HIP(hipDeviceSynchronize()); hipFree(wred_dev); }
        wred_dev = nullptr; wred_cap = 0; wred_sent.clear();
        VR_HIP(hipMalloc(reinterpret_cast<void**>(&wred_dev), 2 * bytes));
        wred_cap = 2 * wred_host.size();
    }
    // the table is the same in every step of a plan (bump-allocated slabs, fixed gradient arena): uploaded only when it changed
    if (wred_sent.size() != wred_host.size() || memcmp(wred_sent.data(), wred_host.data(), bytes) != 0) {
        VR_HIP(hipStreamSynchronize(st));                         // (the previous step's launch may still be reading the old table)
        VR_HIP(hipMemcpy(wred_dev, wred_host.data(), bytes, hipMemcpyHostToDevice));
        wred_sent = wred_host;
    }
    launch_wgrad_reduce_batched(wred_dev, (int)wred_host.size(), blocks, vec, st);
    wred_host.clear();
}

// ---- the train-form head: the one path from the feature tensor f3 to the loss and to the gradients of f3 and of the head weights, for
// the fused step, the split step's backward (launch_head_grads, its "dlogit is given" tail) and the head_* hooks of debug.hip ------------
void launch_head_grads(const Tensor& f3, int CO, const float* w, const float* dlogit, float* wpart, float* g, int g_acc, float* dw,
                       int dw_acc, hipStream_t st) {
    launch_thin_wgrad(f3, CO, dlogit, wpart, dw, dw_acc, st);
    launch_thin_dgrad(f3, CO, w, dlogit, g, g_acc, st);
}

void run_train_head(const FFTPlan& pl, const Tensor& f3, const TrainHead& h, const HeadScratch& s, WaveTable* staging, hipStream_t st) {
    const int CO = h.cplx ? 4 : 2;
    if (h.kind == 0) {
        if (h.cplx) launch_head_loss_complex(f3, h.w, h.X, h.Y, h.bins, h.grad_scale, s.dlogit, h.mask, s.lpart, h.loss, h.loss_scale, st);
        else launch_head_loss(f3, h.w, h.X, h.Y, h.bins, h.grad_scale, s.dlogit, h.mask, s.lpart, h.loss, h.loss_scale, st);
        if (!h.dw) return;
    } else {
        // VR_LOSS_MAG_L1_WAVE_SDR / _WSDR (DESIGN.md sections 6n, 6o): the mask and the magnitude term, the waves and their three or six
        // sums behind it in `loss`, dmask from the sums, dlogit from dmask
        float* mask = h.mask ? h.mask : s.mask;
        launch_head_mag_l1(f3, h.w, h.X, h.Y, h.bins, mask, s.lpart, h.loss, h.loss_scale, st);
        if (!h.dw) return;
        const int signals = f3.N * 2, T = f3.W;
        const float2 *xc = reinterpret_cast<const float2*>(h.X), *yc = reinterpret_cast<const float2*>(h.Y), *mc = reinterpret_cast<const float2*>(mask);
        float2* dm = reinterpret_cast<float2*>(s.dmask);
        if (h.kind == 3) {
            launch_wave_term(pl, WaveTriple{xc, yc, mc, nullptr, T, 0, T, s.wave[2], s.wave[0], s.wave[1], s.part}, s.table, staging, signals, T, h.loss + 1, st);
            launch_stft_wave_grad3(pl, WaveGrad3{s.wave[2], s.wave[0], s.wave[1], h.loss + 1, xc, mc, yc, dm, h.sdr_scale, h.grad_scale}, signals, T, st);
        } else {
            launch_wave_term(pl, WavePair{xc, mc, yc, T, T, 0, s.wave[0], s.wave[1], s.part}, s.table, staging, signals, T, h.loss + 1, st);
            launch_stft_wave_grad(pl, WaveGrad{s.wave[0], s.wave[1], h.loss + 1, xc, mc, yc, dm, h.sdr_scale, h.grad_scale}, signals, T, st);
        }
        launch_head_bwd_complex(f3, h.w, s.dmask, h.bins, s.dlogit, st);
    }
    launch_head_grads(f3, CO, h.w, s.dlogit, s.wpart, h.g, h.g_acc, h.dw, h.dw_acc, st);
}

// The planning block of the two training entry points: `dry_run` (forward + backward on measuring arenas) sizes ws and gs, both grow to
// it (ws by extra_ws bytes more), and the zero ranges of gs (gs_zero_plan; the real pass allocates in the same order) are cleared --
// beside the forward on lanes[0].main (the fused step: gs is only touched from the loss kernels on) or on the main stream.
template <class F>
void Model::plan_train_arenas(F&& dry_run, size_t extra_ws, bool clear_beside) {
    Arena sws = ws, sgs = gs;
    ws.dry = gs.dry = true; ws.base = gs.base = nullptr; ws.off = gs.off = 0; ws.peak = gs.peak = 0;
    dry = true;
    try { dry_run(); }
    catch (...) { dry = false; ws = sws; gs = sgs; tape.clear(); throw; }
    dry = false;
    gs_zero_plan = gs_zero;
    const size_t need_ws = ws.peak + extra_ws, need_gs = gs.peak + 4096;
    ws = sws; gs = sgs;
    ensure_ws(need_ws);
    if (need_gs > gs.cap) {
        VR_HIP(hipStreamSynchronize(stream));
        if (gs.base) VR_HIP(hipFree(gs.base));
        gs.base = nullptr; gs.cap = 0;
        VR_HIP(hipMalloc(reinterpret_cast<void**>(&gs.base), need_gs + (need_gs >> 4)));
        gs.cap = need_gs + (need_gs >> 4);
    }
    ws.reset(); gs.reset();
    if (clear_beside && !lanes.empty()) {
        VR_HIP(hipEventRecord(lanes[0].fork, stream));            // (previous step's consumers of gs are done)
        VR_HIP(hipStreamWaitEvent(lanes[0].main, lanes[0].fork, 0));
        clear_gs_zero_ranges(lanes[0].main);
        VR_HIP(hipEventRecord(lanes[0].join, lanes[0].main));
        gs_clear_pending = true;
    } else {
        wait_gs_clear();
        clear_gs_zero_ranges(stream);
    }
}

void Model::wait_gs_clear() {
    if (gs_clear_pending) { VR_HIP(hipStreamWaitEvent(stream, lanes[0].join, 0)); gs_clear_pending = false; }
}

// what both train-mode entry points do after their checks: the flipped / transposed weights for the data gradients and the Winograd-domain
// copies of both, once per step (before the planning dry run: the kernel choice, hence the partial-statistics layout, depends on them)
void Model::refresh_train_weights() {
    ensure_train_state();
    refresh_forms(true);
}

void Model::train_fwd_bwd_api(const float* X, const float* Y, bool on_dev, int B, int T, int accumulation_steps,
                              float* loss_out, float* mask_out, bool mask_on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(training, -2, "train step needs train mode: call vr_set_mode(h, 1) (model.train(), train.py:69)");
    graph_valid = false;
    VR_CHECK(B > 0 && accumulation_steps > 0, -2, "batch and accumulation_steps must be positive");
    // (so T >= 16: the wave terms of kinds 1 / 3 always have samples)
    VR_CHECK(T > 0 && T % 16 == 0, -5, "h1_shape[3] must be greater than h2_shape[3] (frames must be a multiple of 16)");
    refresh_train_weights();
    // a complex handle ("complex_train"): X, y, mask are interleaved complex64, the network reads four planar channels, the head has four
    // outputs -- every buffer below that holds complex or four-channel data doubles, in the dry run and the real one alike
    const size_t io_floats = (size_t)B * 2 * output_bin * T * (is_complex ? 2 : 1);
    const bool wsdr_loss = loss_kind == 3, wave_loss = loss_kind == 1 || wsdr_loss;      // VR_LOSS_MAG_L1_WAVE_WSDR: DESIGN.md section 6o
    const double ntot = (double)B * 2 * output_bin * T;          // (complex handle: complex elements, as torch's L1Loss counts them)
    auto run_all = [&](const float* xd, const float* yd, float* maskd, float* lossd) {
        tape.clear();
        g_fresh.clear(); gs_zero.clear();
        Tensor f3 = run_net(net_input(xd, nullptr, B, T));
        // head + loss (train.py:81,89) and its backward into f3.g / out.weight; kinds 1 / 3 keep the mask even when the caller does not ask
        // for it (scratch: the dry run, which has no maskd, sizes the same)
        const HeadScratch hs = head_scratch([&](size_t n) { return ws.allocf(n); }, plan, hop, f3, loss_kind, is_complex, output_bin);
        if (!dry) {
            wait_gs_clear();
            const TrainHead h{loss_kind, is_complex, out_w->dev, xd, yd, output_bin, maskd, lossd, (float)(1.0 / ntot),
                              (float)(1.0 / (ntot * accumulation_steps)), (float)(sdr_weight / accumulation_steps),
                              f3.g, g_first(f3.g) ? 0 : 1, grad_of(out_w), 1};
            run_train_head(plan, f3, h, hs, &wave_host, stream);
        }
        backward();
    };
    plan_train_arenas([&] { run_all(reinterpret_cast<float*>(uintptr_t(256)), nullptr, nullptr, nullptr); },
                  (3 * io_floats + 64) * sizeof(float) + 8192, true);
    prepare_dropout(B);
    // ---- inputs ---------------------------------------------------------------------------------------------------
    const float *xd = X, *yd = Y;
    if (!on_dev) {
        float* tx = ws.allocf(io_floats);
        float* ty = ws.allocf(io_floats);
        VR_HIP(hipMemcpyAsync(tx, X, io_floats * sizeof(float), hipMemcpyHostToDevice, stream));
        VR_HIP(hipMemcpyAsync(ty, Y, io_floats * sizeof(float), hipMemcpyHostToDevice, stream));
        xd = tx; yd = ty;
    }
    float* maskd = nullptr;
    if (mask_out) maskd = mask_on_dev ? mask_out : ws.allocf(io_floats);
    float* lossd = ws.allocf(16);

    run_all(xd, yd, maskd, lossd);
    // the loss; VR_LOSS_MAG_L1_WAVE_SDR: its magnitude term and the three wave sums; VR_LOSS_MAG_L1_WAVE_WSDR: the term and six sums
    float l4[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    VR_HIP(hipMemcpyAsync(l4, lossd, (wsdr_loss ? 7 : wave_loss ? 4 : 1) * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (mask_out && !mask_on_dev) VR_HIP(hipMemcpyAsync(mask_out, maskd, io_floats * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    const float loss_h = wsdr_loss ? finish_wsdr_loss(l4) : wave_loss ? finish_wave_loss(l4) : l4[0];
    if (loss_out) *loss_out = loss_h;
    tape.clear();
    affine_dirty = true;
    dropout_dev = nullptr;
}

// ---- the autograd split of the same step: `mask = model(X)` keeps the graph, `loss.backward()` comes later with
// dLoss/dmask (train.py:81,92 as two calls, so that the reference's own loss expression and torch's own optimizer can
// sit in between).  The graph lives in the workspace arenas: any other call on the handle invalidates it. ------------
void Model::forward_train_api(const float* X, bool on_dev, int B, int T, float* mask_out, bool mask_on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(training, -2, "forward with a graph needs train mode: call vr_set_mode(h, 1) (model.train(), train.py:69)");
    VR_CHECK(B > 0, -2, "batch must be positive");
    VR_CHECK(T > 0 && T % 16 == 0, -5, "h1_shape[3] must be greater than h2_shape[3] (frames must be a multiple of 16)");
    VR_CHECK(mask_out != nullptr, -2, "null argument");
    graph_valid = false;
    refresh_train_weights();
    const int CO = is_complex ? 4 : 2;
    const size_t io_floats = (size_t)B * 2 * output_bin * T * (is_complex ? 2 : 1);
    auto fwd = [&](const float* x, const hipMemcpyKind* copy) {
        tape.clear();
        g_fresh.clear(); gs_zero.clear();
        return run_net(net_input(x, copy, B, T));
    };
    plan_train_arenas([&] {
        ws.allocf(3 * io_floats + 64);               // the real run's input copy, graph_mask and 64 floats to spare
        Tensor f3 = fwd(reinterpret_cast<float*>(uintptr_t(256)), nullptr);
        ws.allocf((size_t)B * CO * max_bin * T);     // the allocations backward_api makes, in its order
        ws.allocf((size_t)thin_wgrad_blocks(f3) * CO * f3.C);
        backward();
    }, 8192, false);
    prepare_dropout(B);
    graph_mask = ws.allocf(io_floats);
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    graph_f3 = fwd(X, &kind);
    mask_head(graph_f3, 0, T, graph_mask);
    VR_HIP(hipMemcpyAsync(mask_out, graph_mask, io_floats * sizeof(float), mask_on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    graph_valid = true; graph_B = B; graph_T = T; ++graph_gen;
    affine_dirty = true;
}

void Model::backward_api(const float* dmask, bool on_dev) {
    DeviceGuard dev_guard(device);
    VR_CHECK(graph_valid, -2, "vr_backward: no graph -- call vr_forward_train first (another call on the handle in between frees it)");
    VR_CHECK(dmask != nullptr, -2, "null argument");
    graph_valid = false;
    const int B = graph_B, T = graph_T, Hm = max_bin;
    const int cplx = is_complex ? 2 : 1, CO = 2 * cplx;
    const size_t io_floats = (size_t)B * 2 * output_bin * T * cplx;
    const Tensor& f3 = graph_f3;
    const float* dm = dmask;
    float* tmp = nullptr;
    struct Free { float*& p; hipStream_t s; ~Free() { if (p) { hipStreamSynchronize(s); hipFree(p); } } } fr{tmp, stream};
    if (!on_dev) {                                                 // the input copy of the forward is dead by now: reuse nothing, stage after the tape
        VR_HIP(hipMalloc(&tmp, io_floats * sizeof(float)));
        VR_HIP(hipMemcpyAsync(tmp, dmask, io_floats * sizeof(float), hipMemcpyHostToDevice, stream));
        dm = tmp;
    }
    float* dlogit = ws.allocf((size_t)B * CO * Hm * T);
    float* wpart = ws.allocf((size_t)thin_wgrad_blocks(f3) * CO * f3.C);
    if (is_complex) launch_head_bwd_complex(f3, out_w->dev, dm, output_bin, dlogit, stream);
    else launch_head_bwd(dm, graph_mask, B, Hm, T, output_bin, dlogit, stream);
    launch_head_grads(f3, CO, out_w->dev, dlogit, wpart, f3.g, g_first(f3.g) ? 0 : 1, grad_of(out_w), 1, stream);
    backward();
    VR_HIP(hipStreamSynchronize(stream));
    tape.clear();
    dropout_dev = nullptr;
}

void Model::aug_reserve(size_t need) {
    if (need <= aug_cap) return;
    VR_HIP(hipStreamSynchronize(stream));
    if (aug_buf) VR_HIP(hipFree(aug_buf));
    aug_buf = nullptr; aug_cap = 0;
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&aug_buf), need + (need >> 3)));
    aug_cap = need + (need >> 3);
}

// vr_pipeline_buffer: what the handle holds for the input pipeline (tables, host outputs and, over a wave store, the rows of a batch), and
// its release; the next call that needs it allocates it again
long long Model::pipeline_buffer(bool release) {
    const long long held = (long long)aug_cap;
    if (release && aug_buf) {
        DeviceGuard dev_guard(device);
        VR_HIP(hipStreamSynchronize(stream));
        VR_HIP(hipFree(aug_buf));
        aug_buf = nullptr; aug_cap = 0;
    }
    return held;
}

// What the _ex entry points refuse in a descriptor table, before anything is launched (the rows of a remix partner are checked where
// a mixup partner's are).  -> true when no sample carries a new bit; `plain` then holds the table as AugDesc, and the caller goes the
// way of the old entry point: the same instantiation, so the same bytes.
static bool aug_ex_check(const AugDescEx* d, int B, const char* who, std::vector<AugDesc>& plain) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const int flags = d[b].flags;
        const std::string at = std::string(who) + ": sample " + std::to_string(b) + ": ";
        any = any || (flags & kAugExBits);
        if (!(flags & kAugRemix)) continue;
        VR_CHECK(!(flags & kAugMix), -2, at + "remix and mixup are both flagged; a sample has one partner");
        VR_CHECK(!(flags & (16 | 64)), -2, at + "remix flagged with the partner's " + ((flags & 16) ? "reduce" : "inst-only") +
                                               " bit; a remix partner takes its swap bit only");
        VR_CHECK(std::isfinite(d[b].gain_y), -2, at + "gain_y is not finite");
        VR_CHECK(std::isfinite(d[b].gain_v), -2, at + "gain_v is not finite");
    }
    if (any) return false;
    plain.resize((size_t)B);
    for (int b = 0; b < B; ++b) plain[b] = AugDesc{d[b].coef, d[b].coef_mix, d[b].lam, d[b].flags};
    return true;
}

// Training input pipeline (lib/dataset.py:105-120 after the random draws and the file reads), see augment.hip.
void Model::augment_api(const float* Xc, const float* yc, const float* Xi, const float* yi, const void* desc, const float* rw,
                        int B, int T, int bins, bool in_on_dev, float* Xmag, float* ymag, bool out_on_dev, bool out_complex, bool ex) {
    DeviceGuard dev_guard(device);
    VR_CHECK(B > 0 && T > 0 && bins > 0, -2, "augment: empty batch");
    std::vector<AugDesc> plain;
    if (ex && aug_ex_check(static_cast<const AugDescEx*>(desc), B, "vr_augment_batch_ex", plain)) {       // no new bit: today's launch
        desc = plain.data();
        ex = false;
    }
    const size_t crop_b = (size_t)B * T * 2 * bins * sizeof(float2), out_b = (size_t)B * 2 * bins * T * (out_complex ? sizeof(float2) : sizeof(float));
    const size_t desc_b = (size_t)B * (ex ? sizeof(AugDescEx) : sizeof(AugDesc)), rw_b = (size_t)bins * sizeof(float);
    auto up256 = [](size_t v) { return (v + 255) & ~size_t(255); };
    size_t need = up256(desc_b) + up256(rw_b);
    if (!in_on_dev) need += 4 * up256(crop_b);
    if (!out_on_dev) need += 2 * up256(out_b);
    aug_reserve(need);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = aug_buf + off; off += up256(bytes); return p; };
    char* dd = take(desc_b);
    float* drw = reinterpret_cast<float*>(take(rw_b));
    VR_HIP(hipMemcpyAsync(dd, desc, desc_b, hipMemcpyHostToDevice, stream));
    if (rw) VR_HIP(hipMemcpyAsync(drw, rw, rw_b, hipMemcpyHostToDevice, stream));
    const float* src[4] = {Xc, yc, Xi, yi};
    const float2* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
        if (!src[i]) continue;
        if (in_on_dev) { dev[i] = reinterpret_cast<const float2*>(src[i]); continue; }
        char* p = take(crop_b);
        VR_HIP(hipMemcpyAsync(p, src[i], crop_b, hipMemcpyHostToDevice, stream));
        dev[i] = reinterpret_cast<const float2*>(p);
    }
    float* ox = out_on_dev ? Xmag : reinterpret_cast<float*>(take(out_b));
    float* oy = out_on_dev ? ymag : reinterpret_cast<float*>(take(out_b));
    if (ex)
        launch_augment(dev[0], dev[1], dev[2] ? dev[2] : dev[0], dev[3] ? dev[3] : dev[1], reinterpret_cast<const AugDescEx*>(dd),
                       rw ? drw : nullptr, B, T, bins, ox, oy, out_complex, stream);
    else
        launch_augment(dev[0], dev[1], dev[2] ? dev[2] : dev[0], dev[3] ? dev[3] : dev[1], reinterpret_cast<const AugDesc*>(dd),
                       rw ? drw : nullptr, B, T, bins, ox, oy, out_complex, stream);
    if (!out_on_dev) {
        VR_HIP(hipMemcpyAsync(Xmag, ox, out_b, hipMemcpyDeviceToHost, stream));
        VR_HIP(hipMemcpyAsync(ymag, oy, out_b, hipMemcpyDeviceToHost, stream));
    }
    VR_HIP(hipStreamSynchronize(stream));
}

// ---- the resident training set (vr_dataset_*) ---------------------------------------------------------------------------------
ResidentSet::ResidentSet(int device_, int bins_) : device(device_), bins(bins_) {
    DeviceGuard dev_guard(device);
    VR_HIP(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
}

ResidentSet::ResidentSet(int device_, int n_fft_, int hop_) : device(device_), bins(n_fft_ / 2 + 1), waves(true), n_fft(n_fft_), hop(hop_) {
    DeviceGuard dev_guard(device);
    fft_plan_create(plan, n_fft);
    if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) {
        (void)hipFree(plan.twiddle); (void)hipFree(plan.window);
        throw Error(-1, "vr_dataset_create_waves: hipStreamCreateWithFlags failed");
    }
}

ResidentSet::~ResidentSet() {
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(device);
    if (up) (void)hipStreamSynchronize(up);
    for (Song& s : songs) { (void)hipFree(s.X); (void)hipFree(s.y); }
    if (peak_ws) (void)hipFree(peak_ws);
    if (peak_rows) (void)hipFree(peak_rows);
    if (plan.twiddle) (void)hipFree(plan.twiddle);
    if (plan.window) (void)hipFree(plan.window);
    for (int i = 0; i < 2; ++i) {
        if (stage[i]) (void)hipHostFree(stage[i]);
        if (drained[i]) (void)hipEventDestroy(drained[i]);
    }
    if (up) (void)hipStreamDestroy(up);
    if (prev >= 0) (void)hipSetDevice(prev);
}

// Host -> slab in pieces through two pinned buffers: the source may be a memory map of the cache file, so its pages are touched by a
// plain memcpy (never pinned), and the copy of piece k overlaps the device transfer of piece k - 1.
void ResidentSet::upload(float2* dst, const float* src, size_t n_bytes) {
    for (int i = 0; i < 2; ++i) {
        if (!stage[i]) VR_HIP(hipHostMalloc(reinterpret_cast<void**>(&stage[i]), kPiece, hipHostMallocDefault));
        if (!drained[i]) VR_HIP(hipEventCreateWithFlags(&drained[i], hipEventDisableTiming));
    }
    const char* from = reinterpret_cast<const char*>(src);
    char* to = reinterpret_cast<char*>(dst);
    int k = 0;
    for (size_t off = 0; off < n_bytes; off += kPiece, ++k) {
        const size_t n = n_bytes - off < kPiece ? n_bytes - off : kPiece;
        const int i = k & 1;
        if (k >= 2) VR_HIP(hipEventSynchronize(drained[i]));
        std::memcpy(stage[i], from + off, n);
        VR_HIP(hipMemcpyAsync(to + off, stage[i], n, hipMemcpyHostToDevice, up));
        VR_HIP(hipEventRecord(drained[i], up));
    }
    VR_HIP(hipStreamSynchronize(up));
}

int ResidentSet::add(const float* X, const float* y, long long rows) {
    VR_CHECK(!waves, -2, "vr_dataset_add: this store holds waves (vr_dataset_create_waves): add songs with vr_dataset_add_waves or vr_dataset_add_pcm");
    DeviceGuard dev_guard(device);
    VR_CHECK(rows > 0, -2, "vr_dataset_add: rows must be positive");
    const size_t slab = (size_t)rows * 2 * bins * sizeof(float2);
    const float* src[2] = {X, y};
    float2* dev[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc(reinterpret_cast<void**>(&dev[i]), slab) != hipSuccess) {
            (void)hipGetLastError();                     // the failed allocation is reported here, not by the next launch
            if (dev[0]) (void)hipFree(dev[0]);
            throw Error(-4, "vr_dataset_add: hipMalloc of " + std::to_string(slab) + " bytes failed (song of " + std::to_string(rows) +
                                " rows needs two of them; the store already holds " + std::to_string(bytes) + " bytes in " +
                                std::to_string(songs.size()) + " songs)");
        }
    }
    try {
        for (int i = 0; i < 2; ++i) upload(dev[i], src[i], slab);
    } catch (...) {
        (void)hipFree(dev[0]); (void)hipFree(dev[1]);
        throw;
    }
    songs.push_back(Song{dev[0], dev[1], rows});
    bytes += 2 * (long long)slab;
    return (int)songs.size() - 1;
}

// ---- the wave store (vr_dataset_create_waves) --------------------------------------------------------------------
// Two slabs of one song, allocated and filled as ResidentSet::add does: host memory in bounded pieces through the pinned staging, device
// memory in one copy on the store's stream.  A slab of sample bytes is rounded up to whole 32-bit words (pcm.h reads aligned words).
int ResidentSet::add_slabs(const void* const src[2], const size_t slab[2], bool on_dev, const Song& proto, const char* who) {
    char* dev[2] = {nullptr, nullptr};
    const size_t alloc[2] = {(slab[0] + 3) & ~size_t(3), (slab[1] + 3) & ~size_t(3)};
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc(reinterpret_cast<void**>(&dev[i]), alloc[i]) != hipSuccess) {
            (void)hipGetLastError();
            if (dev[0]) (void)hipFree(dev[0]);
            throw Error(-4, std::string(who) + ": hipMalloc of " + std::to_string(slab[i]) + " bytes failed (song of " + std::to_string(proto.n) +
                                " samples needs " + std::to_string(slab[0]) + " + " + std::to_string(slab[1]) + "; the store already holds " +
                                std::to_string(bytes) + " bytes in " + std::to_string(songs.size()) + " songs)");
        }
    }
    try {
        for (int i = 0; i < 2; ++i) {
            if (!on_dev) { upload(reinterpret_cast<float2*>(dev[i]), static_cast<const float*>(src[i]), slab[i]); continue; }
            VR_HIP(hipMemcpyAsync(dev[i], src[i], slab[i], hipMemcpyDeviceToDevice, up));
            VR_HIP(hipStreamSynchronize(up));
        }
    } catch (...) {
        (void)hipFree(dev[0]); (void)hipFree(dev[1]);
        throw;
    }
    Song s = proto;
    s.X = reinterpret_cast<float2*>(dev[0]);
    s.y = reinterpret_cast<float2*>(dev[1]);
    songs.push_back(s);
    bytes += (long long)(alloc[0] + alloc[1]);
    return (int)songs.size() - 1;
}

int ResidentSet::add_waves(const float* mix, const float* inst, bool on_dev, long long n) {
    VR_CHECK(waves, -2, "vr_dataset_add_waves: this store holds spectrogram rows (vr_dataset_create): add songs with vr_dataset_add");
    VR_CHECK(n > 0 && n / hop < (1LL << 28), -2, "vr_dataset_add_waves: n must be positive (and below 2^28 hops)");
    VR_CHECK(!on_dev || ((reinterpret_cast<uintptr_t>(mix) | reinterpret_cast<uintptr_t>(inst)) & 3) == 0, -2,
             "vr_dataset_add_waves: a device wave must be 4-byte aligned");
    DeviceGuard dev_guard(device);
    Song proto{nullptr, nullptr, 1 + n / hop};
    proto.n = n;
    const void* const src[2] = {mix, inst};
    const size_t slab[2] = {(size_t)2 * n * sizeof(float), (size_t)2 * n * sizeof(float)};
    return add_slabs(src, slab, on_dev, proto, "vr_dataset_add_waves");
}

int ResidentSet::add_pcm(const void* mix, const void* inst, bool on_dev, long long frames, const int* channels, const int* fmt) {
    VR_CHECK(waves, -2, "vr_dataset_add_pcm: this store holds spectrogram rows (vr_dataset_create): add songs with vr_dataset_add");
    VR_CHECK(frames > 0 && frames / hop < (1LL << 28), -2, "vr_dataset_add_pcm: frames must be positive (and below 2^28 hops)");
    Song proto{nullptr, nullptr, 1 + frames / hop};
    proto.n = frames;
    const void* const src[2] = {mix, inst};
    size_t slab[2];
    for (int i = 0; i < 2; ++i) {
        const std::string who = std::string("vr_dataset_add_pcm: ") + (i ? "instrumental: " : "mixture: ");
        VR_CHECK(pcm_fmt_ok(fmt[i]), -2, who + "unknown sample format " + std::to_string(fmt[i]));
        VR_CHECK(channels[i] == 1 || channels[i] == 2, -2, who + "channels must be 1 or 2, got " + std::to_string(channels[i]));
        proto.fmt[i] = fmt[i];
        proto.channels[i] = channels[i];
        slab[i] = (size_t)frames * channels[i] * pcm_sample_bytes(fmt[i]);
    }
    DeviceGuard dev_guard(device);
    // (the device copy starts at the slab's aligned first byte, so a source buffer may lie anywhere, host or device)
    return add_slabs(src, slab, on_dev, proto, "vr_dataset_add_pcm");
}

CropSeg ResidentSet::crop_seg(int song, int which, long long start, int T, float2* dst) const {
    const Song& s = songs[song];
    return CropSeg{which ? static_cast<const void*>(s.y) : static_cast<const void*>(s.X), s.n, start, dst, T, s.fmt[which], s.channels[which], 0};
}

// vr_dataset_peak of a wave store: the song's rows pass through the store's own scratch kPeakChunkRows at a time -- one crop launch for
// both slabs, then the two launches of launch_song_peak on that chunk -- and the chunk candidates are merged here by the kernel's rule: the
// larger key, ties to the lowest (slab, index).  Every chunk's candidate is copied to its own host slot; one wait at the end.
float ResidentSet::peak_waves(int song, float* at, int* slab, long long* index) {
    DeviceGuard dev_guard(device);
    const Song& s = songs[song];
    auto up256 = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t chunk_b = up256((size_t)kPeakChunkRows * 2 * bins * sizeof(float2)), tab_b = up256(2 * sizeof(CropSeg));
    const size_t cand_b = up256((size_t)(kPeakParts + 1) * sizeof(PeakCand));
    if (!peak_rows) {
        const size_t ws_bytes = 2 * chunk_b + tab_b + cand_b;
        if (hipMalloc(reinterpret_cast<void**>(&peak_rows), ws_bytes) != hipSuccess) {
            (void)hipGetLastError();
            peak_rows = nullptr;
            throw Error(-4, "vr_dataset_peak: hipMalloc of " + std::to_string(ws_bytes) + " bytes of scratch failed (the store holds " +
                                std::to_string(bytes) + " bytes in " + std::to_string(songs.size()) + " songs)");
        }
    }
    float2* rx = reinterpret_cast<float2*>(peak_rows);
    float2* ry = reinterpret_cast<float2*>(peak_rows + chunk_b);
    CropSeg* tab = reinterpret_cast<CropSeg*>(peak_rows + 2 * chunk_b);
    PeakCand* cand_dev = reinterpret_cast<PeakCand*>(peak_rows + 2 * chunk_b + tab_b);
    const int chunks = (int)((s.rows + kPeakChunkRows - 1) / kPeakChunkRows);
    std::vector<PeakCand> cand((size_t)chunks);
    std::vector<CropSeg> segs((size_t)chunks * 2);
    for (int c = 0; c < chunks; ++c) {
        const long long r0 = (long long)c * kPeakChunkRows;
        const int T = (int)std::min<long long>(kPeakChunkRows, s.rows - r0);
        segs[2 * c] = crop_seg(song, 0, r0, T, rx);
        segs[2 * c + 1] = crop_seg(song, 1, r0, T, ry);
        VR_HIP(hipMemcpyAsync(tab, &segs[2 * c], 2 * sizeof(CropSeg), hipMemcpyHostToDevice, up));
        launch_stft_crops(plan, tab, 2, T, 2.0 * T, up);
        const long long n = (long long)T * 2 * bins;
        launch_song_peak(rx, ry, n, cand_dev, up);
        VR_HIP(hipMemcpyAsync(&cand[c], cand_dev + song_peak_parts(n), sizeof(PeakCand), hipMemcpyDeviceToHost, up));
    }
    VR_HIP(hipStreamSynchronize(up));
    bool bad = false, have = false;
    float key = -1.f, re = 0.f, im = 0.f;
    // (no candidate at all -- every element NaN: slab and index as the rows store derives them from the kernel's empty position ~0)
    int best_slab = 1;
    long long best_index = -1 - s.rows * 2 * bins;
    for (int c = 0; c < chunks; ++c) {
        const long long r0 = (long long)c * kPeakChunkRows;
        const long long n = std::min<long long>(kPeakChunkRows, s.rows - r0) * 2 * bins;
        const PeakCand& r = cand[c];
        bad = bad || r.bad;
        if (r.pos >= 2ull * (unsigned long long)n) continue;                     // (every element of the chunk NaN: no candidate)
        const int sl = r.pos >= (unsigned long long)n ? 1 : 0;
        const long long idx = r0 * 2 * bins + (long long)(sl ? r.pos - (unsigned long long)n : r.pos);
        const bool wins = !have || r.key > key || (r.key == key && (sl < best_slab || (sl == best_slab && idx < best_index)));
        if (wins) { have = true; key = r.key; re = r.re; im = r.im; best_slab = sl; best_index = idx; }
    }
    if (at) { at[0] = re; at[1] = im; }
    if (slab) *slab = best_slab;
    if (index) *index = best_index;
    return bad ? std::numeric_limits<float>::quiet_NaN() : numpy_cabsf(re, im);
}

// The peak of one song from its resident rows: two launches on the store's stream (augment.hip, SongPeak), one candidate back.  The
// float is formed here, from the one element the device reports, by the operations numpy's np.abs performs on a complex64.
float ResidentSet::peak(int song, float* at, int* slab, long long* index) {
    VR_CHECK(song >= 0 && song < (int)songs.size(), -2, "vr_dataset_peak: song " + std::to_string(song) + " out of range (the dataset holds " +
                                                            std::to_string(songs.size()) + ")");
    if (waves) return peak_waves(song, at, slab, index);
    DeviceGuard dev_guard(device);
    const Song& s = songs[song];
    const long long n = s.rows * 2 * bins;
    const int parts = song_peak_parts(n);
    VR_CHECK(parts >= 1 && parts <= kPeakParts, -1, "vr_dataset_peak: " + std::to_string(parts) + " partials for a workspace of " +
                                                        std::to_string(kPeakParts));
    if (!peak_ws) {
        const size_t ws_bytes = (size_t)(kPeakParts + 1) * sizeof(PeakCand);
        if (hipMalloc(reinterpret_cast<void**>(&peak_ws), ws_bytes) != hipSuccess) {
            (void)hipGetLastError();
            peak_ws = nullptr;
            throw Error(-4, "vr_dataset_peak: hipMalloc of " + std::to_string(ws_bytes) + " bytes failed (the store holds " +
                                std::to_string(bytes) + " bytes in " + std::to_string(songs.size()) + " songs)");
        }
    }
    launch_song_peak(s.X, s.y, n, peak_ws, up);
    PeakCand r;
    VR_HIP(hipMemcpyAsync(&r, peak_ws + parts, sizeof(PeakCand), hipMemcpyDeviceToHost, up));
    VR_HIP(hipStreamSynchronize(up));
    if (at) { at[0] = r.re; at[1] = r.im; }
    if (slab) *slab = r.pos >= (unsigned long long)n ? 1 : 0;
    if (index) *index = (long long)(r.pos >= (unsigned long long)n ? r.pos - (unsigned long long)n : r.pos);
    return r.bad ? std::numeric_limits<float>::quiet_NaN() : numpy_cabsf(r.re, r.im);
}

// (wave store) what a handle must share with the store before it may cut anything from it: the transform's two sizes
void Model::wave_store_check(const ResidentSet& set, const char* who, int B) const {
    VR_CHECK(n_fft == set.n_fft && hop == set.hop, -2,
             std::string(who) + ": the handle transforms at n_fft " + std::to_string(n_fft) + ", hop_length " + std::to_string(hop) +
                 ", the wave store was created for n_fft " + std::to_string(set.n_fft) + ", hop_length " + std::to_string(set.hop));
    VR_CHECK(B <= 16383, -2, std::string(who) + ": at most 16383 samples per call on a wave store (four table entries each)");
}

// Windows of resident songs (vr_dataset_windows): every entry is checked on the host, the table goes to the handle's aug_buf in one copy
// and the SongWindows form of augment_kernel reads the rows where they lie.  A window may leave its song on either side (those rows are
// zero), so the checks are the song index, start + T as an int64, and a finite scale.
void Model::dataset_windows_api(const ResidentSet& set, const ResidentWindow* w, int B, int T, float* Xmag, float* ymag, bool out_on_dev,
                                bool out_complex) {
    VR_CHECK(set.device == device, -2, "vr_dataset_windows: the handle is on device " + std::to_string(device) + ", the dataset on device " +
                                           std::to_string(set.device));
    VR_CHECK(T > 0, -2, "vr_dataset_windows: T must be positive");
    if (set.waves) wave_store_check(set, "vr_dataset_windows", B);
    const int bins = set.bins, n_songs = (int)set.songs.size();
    auto up256 = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t tab_b = (size_t)B * sizeof(SongWindow), head = up256(tab_b);
    const size_t out_b = (size_t)B * 2 * bins * T * (out_complex ? sizeof(float2) : sizeof(float));
    std::vector<SongWindow> tab((size_t)B);
    std::vector<CropSeg> segs;                           // (wave store) two entries per window that meets its song
    std::vector<int> seg_of;                             // ... and the sample each pair belongs to
    for (int b = 0; b < B; ++b) {
        const std::string who = "vr_dataset_windows: sample " + std::to_string(b) + ": ";
        VR_CHECK(w[b].song >= 0 && w[b].song < n_songs, -2, who + "song " + std::to_string(w[b].song) + " out of range (the dataset holds " +
                                                               std::to_string(n_songs) + ")");
        VR_CHECK(w[b].start <= std::numeric_limits<long long>::max() - T, -2, who + "start " + std::to_string(w[b].start) + " + T " +
                                                                                 std::to_string(T) + " overflows");
        VR_CHECK(std::isfinite(w[b].scale), -2, who + "scale " + std::to_string(w[b].scale) + " is not finite");
        const ResidentSet::Song& s = set.songs[w[b].song];
        tab[b] = SongWindow{s.X, s.y, s.rows, w[b].start, w[b].scale, 0};
        if (set.waves) {
            // the rows of the window that lie inside the song, [lo, hi), are formed in scratch; the entry then describes a song of hi - lo
            // rows that the window meets at start - lo, so the rows outside stay the kernel's zeros
            const long long lo = std::max<long long>(w[b].start, 0), hi = std::min<long long>(w[b].start + T, s.rows);
            tab[b] = SongWindow{nullptr, nullptr, std::max<long long>(hi - lo, 0), w[b].start - lo, w[b].scale, 0};
            if (hi > lo) {
                seg_of.push_back(b);
                segs.push_back(set.crop_seg(w[b].song, 0, lo, (int)(hi - lo), nullptr));
                segs.push_back(set.crop_seg(w[b].song, 1, lo, (int)(hi - lo), nullptr));
            }
        }
    }
    DeviceGuard dev_guard(device);
    const size_t out_all = out_on_dev ? 0 : 2 * up256(out_b);
    const size_t seg_b = up256(segs.size() * sizeof(CropSeg)), rows_b = up256((size_t)T * 2 * bins * sizeof(float2));
    // (wave store) reserved for the most the call's B and T can need -- both slabs of every window -- so that the buffer's size follows
    // from B and T alone and a later call of the same shape never grows it
    aug_reserve(head + out_all + (set.waves ? up256((size_t)2 * B * sizeof(CropSeg)) + (size_t)2 * B * rows_b : 0));
    if (!segs.empty()) {
        char* scratch = aug_buf + head + out_all + seg_b;
        int max_T = 0;
        double rows_total = 0.0;
        for (size_t e = 0; e < segs.size(); ++e) {
            segs[e].dst = reinterpret_cast<float2*>(scratch + e * rows_b);
            max_T = std::max(max_T, segs[e].T);
            rows_total += segs[e].T;
            if (e & 1) { tab[seg_of[e >> 1]].X = segs[e - 1].dst; tab[seg_of[e >> 1]].y = segs[e].dst; }
        }
        CropSeg* dseg = reinterpret_cast<CropSeg*>(aug_buf + head + out_all);
        VR_HIP(hipMemcpyAsync(dseg, segs.data(), segs.size() * sizeof(CropSeg), hipMemcpyHostToDevice, stream));
        launch_stft_crops(set.plan, dseg, (int)segs.size(), max_T, rows_total, stream);
    }
    VR_HIP(hipMemcpyAsync(aug_buf, tab.data(), tab_b, hipMemcpyHostToDevice, stream));
    float* ox = out_on_dev ? Xmag : reinterpret_cast<float*>(aug_buf + head);
    float* oy = out_on_dev ? ymag : reinterpret_cast<float*>(aug_buf + head + up256(out_b));
    prof_note(0.0, (out_complex ? 32.0 : 24.0) * (double)B * 2 * bins * T);
    launch_song_windows(reinterpret_cast<const SongWindow*>(aug_buf), B, T, bins, ox, oy, out_complex, stream);
    if (!out_on_dev) {
        VR_HIP(hipMemcpyAsync(Xmag, ox, out_b, hipMemcpyDeviceToHost, stream));
        VR_HIP(hipMemcpyAsync(ymag, oy, out_b, hipMemcpyDeviceToHost, stream));
    }
    VR_HIP(hipStreamSynchronize(stream));
}

// One batch cut from the store: the host checks every crop against its song (the kernel is never given a row it cannot read), then
// pointer table, descriptors and reduction weight go to the handle's aug_buf in ONE copy and augment_kernel<true> reads the crops
// where they lie.
void Model::dataset_batch_api(const ResidentSet& set, const ResidentCrop* crops, const void* desc, const float* rw, int B, int T,
                              float* Xmag, float* ymag, bool out_on_dev, bool out_complex, bool ex) {
    VR_CHECK(set.device == device, -2, "vr_dataset_batch: the handle is on device " + std::to_string(device) + ", the dataset on device " +
                                           std::to_string(set.device));
    VR_CHECK(T > 0, -2, "vr_dataset_batch: T must be positive");
    if (set.waves) wave_store_check(set, "vr_dataset_batch", B);
    std::vector<AugDesc> plain;
    if (ex && aug_ex_check(static_cast<const AugDescEx*>(desc), B, "vr_dataset_batch_ex", plain)) {       // no new bit: today's launch
        desc = plain.data();
        ex = false;
    }
    // (ex) the table is read through its stride; a partner is a mixup partner or a remix partner
    const size_t desc_sz = ex ? sizeof(AugDescEx) : sizeof(AugDesc);
    const int partner = ex ? (kAugMix | kAugRemix) : kAugMix;
    auto flags_of = [&](int b) { return reinterpret_cast<const AugDesc*>(static_cast<const char*>(desc) + (size_t)b * desc_sz)->flags; };
    const int bins = set.bins, n_songs = (int)set.songs.size();
    std::vector<char> host;
    auto up256 = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t tab_b = (size_t)B * sizeof(AugCrops), desc_b = (size_t)B * desc_sz, rw_b = (size_t)bins * sizeof(float);
    const size_t out_b = (size_t)B * 2 * bins * T * (out_complex ? sizeof(float2) : sizeof(float));
    const size_t head = up256(tab_b) + up256(desc_b) + (rw ? up256(rw_b) : 0);
    host.resize(head);
    AugCrops* tab = reinterpret_cast<AugCrops*>(host.data());
    std::vector<CropSeg> segs;                           // (wave store) launch 1's table: X, y and, with bit 3, the partners of every sample
    std::vector<int> first((size_t)(set.waves ? B : 0)); // ... and each sample's first entry in it
    auto rows_at = [&](int b, const char* which, int song, long long start) -> size_t {
        const std::string who = "vr_dataset_batch: sample " + std::to_string(b) + ": " + which;
        VR_CHECK(song >= 0 && song < n_songs, -2, who + "song " + std::to_string(song) + " out of range (the dataset holds " +
                                                     std::to_string(n_songs) + ")");
        const long long rows = set.songs[song].rows;
        VR_CHECK(start >= 0, -2, who + "start " + std::to_string(start) + " is negative");
        VR_CHECK(T <= rows && start <= rows - T, -2, who + "rows [" + std::to_string(start) + ", " + std::to_string(start + T) + ") end past the " +
                                                        std::to_string(rows) + " rows of song " + std::to_string(song));
        return (size_t)start * 2 * bins;
    };
    for (int b = 0; b < B; ++b) {
        const int flags = flags_of(b);
        VR_CHECK(!(flags & (1 | 16)) || rw, -2, "vr_dataset_batch: sample " + std::to_string(b) +
                                                   ": vocal reduction flagged but no reduction_weight given");
        const size_t o = rows_at(b, "", crops[b].song, crops[b].start);
        const ResidentSet::Song& s = set.songs[crops[b].song];
        tab[b] = AugCrops{s.X + o, s.y + o, s.X + o, s.y + o};
        if (set.waves) {                                 // (the pointers are set below, once the scratch is reserved)
            first[b] = (int)segs.size();
            segs.push_back(set.crop_seg(crops[b].song, 0, crops[b].start, T, nullptr));
            segs.push_back(set.crop_seg(crops[b].song, 1, crops[b].start, T, nullptr));
        }
        if (flags & partner) {
            const bool remix = ex && (flags & kAugRemix);
            VR_CHECK(crops[b].mix_song >= 0, -2, "vr_dataset_batch: sample " + std::to_string(b) + (remix ? ": remix" : ": mixup") +
                                                     " flagged but mix_song is " + std::to_string(crops[b].mix_song));
            const size_t om = rows_at(b, remix ? "remix partner: " : "mixup partner: ", crops[b].mix_song, crops[b].mix_start);
            const ResidentSet::Song& m = set.songs[crops[b].mix_song];
            tab[b].X_mix = m.X + om;
            tab[b].y_mix = m.y + om;
            if (set.waves) {
                segs.push_back(set.crop_seg(crops[b].mix_song, 0, crops[b].mix_start, T, nullptr));
                segs.push_back(set.crop_seg(crops[b].mix_song, 1, crops[b].mix_start, T, nullptr));
            }
        }
    }
    std::memcpy(host.data() + up256(tab_b), desc, desc_b);
    if (rw) std::memcpy(host.data() + up256(tab_b) + up256(desc_b), rw, rw_b);

    DeviceGuard dev_guard(device);
    const size_t out_all = out_on_dev ? 0 : 2 * up256(out_b);
    const size_t seg_b = up256(segs.size() * sizeof(CropSeg)), rows_b = up256((size_t)T * 2 * bins * sizeof(float2));
    // (wave store) reserved for the most the call's B and T can need -- four signals a sample and the reduction weight, whatever the flags
    // of this batch -- so that the buffer's size follows from B and T alone and a later batch with more partners never grows it
    aug_reserve(set.waves ? up256(tab_b) + up256(desc_b) + up256(rw_b) + out_all + up256((size_t)4 * B * sizeof(CropSeg)) + (size_t)4 * B * rows_b
                          : head + out_all);
    if (set.waves) {
        // launch 1: the crop-table STFT writes every signal's T rows into the handle's scratch; launch 2 below reads them through the
        // AugCrops table exactly as it reads the slabs of a rows store
        char* scratch = aug_buf + head + out_all + seg_b;
        for (size_t e = 0; e < segs.size(); ++e) segs[e].dst = reinterpret_cast<float2*>(scratch + e * rows_b);
        for (int b = 0; b < B; ++b) {
            const int e = first[b], em = (flags_of(b) & partner) ? e + 2 : e;
            tab[b] = AugCrops{segs[e].dst, segs[e + 1].dst, segs[em].dst, segs[em + 1].dst};
        }
        CropSeg* dseg = reinterpret_cast<CropSeg*>(aug_buf + head + out_all);
        VR_HIP(hipMemcpyAsync(dseg, segs.data(), segs.size() * sizeof(CropSeg), hipMemcpyHostToDevice, stream));
        launch_stft_crops(set.plan, dseg, (int)segs.size(), T, (double)segs.size() * T, stream);
    }
    VR_HIP(hipMemcpyAsync(aug_buf, host.data(), head, hipMemcpyHostToDevice, stream));
    const AugCrops* dtab = reinterpret_cast<const AugCrops*>(aug_buf);
    const char* dd = aug_buf + up256(tab_b);
    const float* drw = rw ? reinterpret_cast<const float*>(aug_buf + up256(tab_b) + up256(desc_b)) : nullptr;
    float* ox = out_on_dev ? Xmag : reinterpret_cast<float*>(aug_buf + head);
    float* oy = out_on_dev ? ymag : reinterpret_cast<float*>(aug_buf + head + up256(out_b));
    if (ex) launch_augment_resident(dtab, reinterpret_cast<const AugDescEx*>(dd), drw, B, T, bins, ox, oy, out_complex, stream);
    else launch_augment_resident(dtab, reinterpret_cast<const AugDesc*>(dd), drw, B, T, bins, ox, oy, out_complex, stream);
    if (!out_on_dev) {
        VR_HIP(hipMemcpyAsync(Xmag, ox, out_b, hipMemcpyDeviceToHost, stream));
        VR_HIP(hipMemcpyAsync(ymag, oy, out_b, hipMemcpyDeviceToHost, stream));
    }
    VR_HIP(hipStreamSynchronize(stream));
}

void Model::reset_adam_state() {
    DeviceGuard dev_guard(device);
    adam_step = 0;
    if (m_arena) {
        prof_memset_async(m_arena, 0, p_floats * sizeof(float), stream);
        prof_memset_async(v_arena, 0, p_floats * sizeof(float), stream);
        VR_HIP(hipStreamSynchronize(stream));
    }
}

void Model::adam_step_api(double lr, double b1, double b2, double eps, double grad_scale) {
    DeviceGuard dev_guard(device);
    ensure_train_state();
    adam_step += 1;
    launch_adam(p_arena, g_arena, m_arena, v_arena, (long long)p_floats, lr, b1, b2, eps, adam_step, grad_scale, stream);
    VR_HIP(hipStreamSynchronize(stream));
    affine_dirty = true;
}

void Model::adam_state(float* m_host, float* v_host, int64_t numel, int64_t* step, bool set) {
    DeviceGuard dev_guard(device);
    ensure_train_state();
    VR_CHECK(numel == (int64_t)p_floats, -2, "adam state: element count must equal vr_grad_arena's");
    VR_HIP(hipStreamSynchronize(stream));
    if (set) {
        VR_HIP(hipMemcpy(m_arena, m_host, p_floats * sizeof(float), hipMemcpyHostToDevice));
        VR_HIP(hipMemcpy(v_arena, v_host, p_floats * sizeof(float), hipMemcpyHostToDevice));
        adam_step = *step;
    } else {
        VR_HIP(hipMemcpy(m_host, m_arena, p_floats * sizeof(float), hipMemcpyDeviceToHost));
        VR_HIP(hipMemcpy(v_host, v_arena, p_floats * sizeof(float), hipMemcpyDeviceToHost));
        *step = adam_step;
    }
}

void Model::get_grad(const std::string& key, float* host, int64_t cap_bytes) {
    auto it = by_key.find(key);
    VR_CHECK(it != by_key.end(), -2, "unknown parameter key: " + key);
    Param& p = *it->second;
    VR_CHECK(p.trainable, -2, key + " is a buffer, it has no gradient");
    DeviceGuard dev_guard(device);
    ensure_train_state();
    VR_HIP(hipStreamSynchronize(stream));
    VR_CHECK((size_t)cap_bytes >= p.numel * sizeof(float), -2, "buffer too small for " + key);
    const float* g = g_arena + (p.dev - p_arena);
    if (p.kind == PK_CONV) {
        std::vector<float> tmp((size_t)p.Cin * p.KK * p.CoutPad);
        VR_HIP(hipMemcpy(tmp.data(), g, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int co = 0; co < p.Cout; ++co)
            for (int ci = 0; ci < p.Cin; ++ci)
                for (int k = 0; k < p.KK; ++k)
                    host[((size_t)co * p.Cin + ci) * p.KK + k] = tmp[((size_t)ci * p.KK + k) * p.CoutPad + co];
    } else if (p.kind == PK_LSTM_IH) {
        std::vector<float> tmp((size_t)p.Cin * p.Cout);
        VR_HIP(hipMemcpy2D(tmp.data(), (size_t)p.Cout * sizeof(float), g + p.co_off, (size_t)p.CoutPad * sizeof(float),
                           (size_t)p.Cout * sizeof(float), (size_t)p.Cin, hipMemcpyDeviceToHost));
        for (int co = 0; co < p.Cout; ++co)
            for (int ci = 0; ci < p.Cin; ++ci) host[(size_t)co * p.Cin + ci] = tmp[(size_t)ci * p.Cout + co];
    } else {
        VR_HIP(hipMemcpy(host, g, p.numel * sizeof(float), hipMemcpyDeviceToHost));
    }
}

}  // namespace vr

// =====================================================================================================
// unit-test hook: backward of ONE conv (no BatchNorm) through the MFMA dgrad / wgrad kernels
// =====================================================================================================
namespace vr {

void Model::debug_dgrad_weight_forms(LocalConv& lc) {
    Conv& L = lc.L;
    L.cls = form_class(L.KS, L.stride, L.dh, L.dw, true);    // (the hook takes any 1x1 stride-1 conv for a conv_x3d layer)
    // Where the hook differs from the handle: the Winograd and plane forms of wt are made only under option train_winograd (the handle
    // makes them always and masks them at the launch), the bf16 planes of its U never.
    const std::vector<Conv*> one{&L};
    for (FormId f : {F_WT, F_S2W, F_WINOT, F_WINOT6, F_X3T}) {
        const FormSpec sp = form_spec(f, L, mfma_mode, W6_NONE);
        if (!(sp.held && sp.live && (f == F_WT || f == F_S2W || train_wino))) continue;
        hold_form(f, one, W6_NONE, lc.store);
        fill_form(f, one, W6_NONE, lc.store, true);
    }
}

void Model::debug_conv_bwd(const float* x, int N, int Cin, int H, int W, const float* w_oihw, int Cout, int KS, int stride,
                           int dh, int dw, int up, const float* aff, float slope, const float* dz, float* dx_out,
                           float* dw_out) {
    DeviceGuard dev_guard(device);
    ensure_train_state();
    const int KK = KS * KS, CoutPad = (Cout + 31) / 32 * 32;
    LocalConv lc;
    Conv& L = lc.L;
    Param& P = lc.P;
    L.name = "debug"; L.Cin = Cin; L.Cout = Cout; L.CoutPad = CoutPad; L.KS = KS; L.stride = stride; L.dh = dh; L.dw = dw;
    L.pad_h = KS == 1 ? 0 : dh; L.pad_w = KS == 1 ? 0 : dw; L.bn = nullptr; L.slope = 1.f;
    P.kind = PK_CONV; P.Cin = Cin; P.Cout = Cout; P.KK = KK; P.CoutPad = CoutPad;
    const int Hin = up ? 2 * H : H, Win = up ? 2 * W : W;
    const int Hout = (Hin + 2 * L.pad_h - dh * (KS - 1) - 1) / stride + 1, Wout = (Win + 2 * L.pad_w - dw * (KS - 1) - 1) / stride + 1;
    std::vector<float> wk((size_t)Cin * KK * CoutPad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < KK; ++k) wk[((size_t)ci * KK + k) * CoutPad + co] = w_oihw[((size_t)co * Cin + ci) * KK + k];
    const size_t xin = (size_t)N * Cin * H * W, xout = (size_t)N * Cout * Hout * Wout;
    float *dx, *dgx, *dwk, *dgw, *dzd, *daff = nullptr;
    VR_HIP(hipMalloc(&dx, xin * 4)); VR_HIP(hipMalloc(&dgx, xin * 4)); VR_HIP(hipMalloc(&dwk, wk.size() * 4));
    VR_HIP(hipMalloc(&dgw, wk.size() * 4)); VR_HIP(hipMalloc(&dzd, xout * 4));
    VR_HIP(hipMemcpy(dx, x, xin * 4, hipMemcpyHostToDevice));
    VR_HIP(hipMemset(dgx, 0, xin * 4)); VR_HIP(hipMemset(dgw, 0, wk.size() * 4));
    VR_HIP(hipMemcpy(dwk, wk.data(), wk.size() * 4, hipMemcpyHostToDevice));
    VR_HIP(hipMemcpy(dzd, dz, xout * 4, hipMemcpyHostToDevice));
    if (aff) { VR_HIP(hipMalloc(&daff, (size_t)Cin * 8)); VR_HIP(hipMemcpy(daff, aff, (size_t)Cin * 8, hipMemcpyHostToDevice)); }
    P.dev = dwk; P.grad_override = dgw;
    debug_dgrad_weight_forms(lc);
    Tensor t;
    t.p = dx; t.g = dgx; t.N = N; t.C = Cin; t.H = H; t.W = W; t.sH = W; t.sC = (long long)H * W; t.sN = t.sC * Cin;
    t.aff0 = daff; t.slope = slope;
    TapeRec r;
    r.kind = TK_CONV; r.L = &L; r.N = N;
    SrcSpec sp{t}; sp.up = up != 0;
    r.srcs = {sp};
    r.out.p = nullptr; r.out.g = dzd; r.out.N = N; r.out.C = Cout; r.out.H = Hout; r.out.W = Wout;
    r.out.sH = Wout; r.out.sC = (long long)Hout * Wout; r.out.sN = r.out.sC * Cout; r.out.slope = 1.f;
    {   // size the workspace with a dry pass
        Arena sws = ws;
        ws.dry = true; ws.base = nullptr; ws.off = 0; ws.peak = 0; dry = true;
        try { bwd_conv(r); } catch (...) { dry = false; ws = sws; throw; }
        dry = false;
        const size_t need = ws.peak + 4096;
        ws = sws;
        ensure_ws(need);
        ws.reset();
    }
    bwd_conv(r);
    VR_HIP(hipStreamSynchronize(stream));
    if (wgrad_on_side) { VR_HIP(hipStreamSynchronize(side_stream)); wgrad_on_side = false; }   // the weight gradient ran there
    VR_HIP(hipMemcpy(dx_out, dgx, xin * 4, hipMemcpyDeviceToHost));
    std::vector<float> gk(wk.size());
    VR_HIP(hipMemcpy(gk.data(), dgw, gk.size() * 4, hipMemcpyDeviceToHost));
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int k = 0; k < KK; ++k) dw_out[((size_t)co * Cin + ci) * KK + k] = gk[((size_t)ci * KK + k) * CoutPad + co];
    hipFree(dx); hipFree(dgx); hipFree(dwk); hipFree(dgw); hipFree(dzd); hipFree(daff);
}

}  // namespace vr
